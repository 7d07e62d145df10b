"""The `transitions` contract restated in plain sequential Python on tests/passages_restated.py:
the passages, each work's sequence of unit-bearing passages, the steps between neighbours, the
cells, the keep rule, the per-unit figures and the bytes of the two CSVs.  The oracle of
tests/test_transitions_host.py and tests/test_gpu_transitions.py and of the committed
tests/golden/transitions_*.csv.  The product never imports it."""

import csv
import io

from tests import companions_restated as cr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
CELL_FIELDS = ['FROM', 'TO', 'FROM_FIRST_WORD_INDEX', 'FROM_LAST_WORD_INDEX', 'FROM_CHARACTER',
               'FROM_SCENE', 'TO_FIRST_WORD_INDEX', 'TO_LAST_WORD_INDEX', 'TO_CHARACTER',
               'TO_SCENE', 'STEPS', 'ADVANCES', 'WORKS', 'SHARE_PERCENT', 'LIFT_PERMILLE',
               'DIRECTION', 'FIRST_FAN_WORK_FILENAME', 'FROM_TEXT', 'TO_TEXT']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'PASSAGES',
               'WORKS', 'STARTS', 'ENDS', 'STEPS_OUT', 'STEPS_IN', 'SUCCESSORS', 'PREDECESSORS',
               'BEST_NEXT', 'BEST_NEXT_STEPS', 'TEXT']
UNIT_KEYS = ['passages', 'works', 'starts', 'ends', 'steps_out', 'steps_in', 'successors',
             'predecessors', 'best_next', 'best_steps']
CELL_KEYS = ['a', 'b', 'steps', 'advances', 'works', 'first_work', 'steps_out_a', 'steps_in_b']


def sequence(records, unit_of, min_words=6, max_gap=0):
    """The unit-bearing passages in record order: dicts of work, fan_first, fan_last, orig_first,
    orig_last and unit."""
    recs = [tuple(r[:3]) + (0.0, 0.0) for r in records]      # (distances play no part)
    out = []
    for p in pr.passages(recs, min_words, max_gap):          # (raises on unsorted records)
        a, b = recs[p['first']], recs[p['first'] + p['n_words'] - 1]
        if unit_of[a[2]] != NONE:
            out.append(dict(work=a[0], fan_first=a[1], fan_last=b[1], orig_first=a[2],
                            orig_last=b[2], unit=unit_of[a[2]]))
    return out


def transitions(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0,
                within=NONE, min_steps=1, min_step_works=2, min_share=0):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).
    Returns (one dict of UNIT_KEYS per unit, one dict of CELL_KEYS per kept cell in (a, b)
    order)."""
    if min_words < 1 or min_steps < 1 or min_step_works < 1 or not 0 <= min_share <= 100:
        raise ValueError("min_words, min_steps and min_step_works at least 1, min_share 0 to 100")
    if len(records) >= 1 << 32:
        raise NotImplementedError("too many records")
    units = [dict(passages=0, works=0, starts=0, ends=0, steps_out=0, steps_in=0, successors=0,
                  predecessors=0, best_next=NONE, best_steps=0) for _ in range(n_units)]
    if not records or not n_units:
        return units, []
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    seq = sequence(records, unit_of, min_words, max_gap)
    unit_works = [set() for _ in range(n_units)]
    cells = {}
    for k, p in enumerate(seq):
        u = units[p['unit']]
        u['passages'] += 1
        unit_works[p['unit']].add(p['work'])
        if k == 0 or seq[k - 1]['work'] != p['work']:
            u['starts'] += 1
        if k + 1 == len(seq) or seq[k + 1]['work'] != p['work']:
            u['ends'] += 1
            continue
        q = seq[k + 1]
        if within != NONE and q['fan_first'] - p['fan_last'] > within + 1:
            continue
        c = cells.setdefault((p['unit'], q['unit']), dict(steps=0, advances=0, works=set()))
        c['steps'] += 1
        c['advances'] += 1 if q['orig_first'] > p['orig_last'] else 0
        c['works'].add(p['work'])
        u['steps_out'] += 1
        units[q['unit']]['steps_in'] += 1
    for u, works in zip(units, unit_works):
        u['works'] = len(works)
    out = []
    for (a, b) in sorted(cells):
        c = cells[(a, b)]
        steps = c['steps']
        if (steps < min_steps or len(c['works']) < min_step_works
                or steps * 100 < min_share * units[a]['steps_out']):
            continue
        out.append(dict(a=a, b=b, steps=steps, advances=c['advances'], works=len(c['works']),
                        first_work=min(c['works']), steps_out_a=units[a]['steps_out'],
                        steps_in_b=units[b]['steps_in']))
        units[a]['successors'] += 1
        units[b]['predecessors'] += 1
        # the most steps, the smaller b on a tie ((a, b) ascends: the first of equals stays)
        if steps > units[a]['best_steps']:
            units[a]['best_next'], units[a]['best_steps'] = b, steps
    return units, out


def share_percent(steps, steps_out):
    return steps * 100 // steps_out


def lift_permille(steps, total_steps, steps_out, steps_in):
    """1000: what choosing the next stretch independently of the current one would give."""
    return steps * total_steps * 1000 // (steps_out * steps_in)


def direction(a, b):
    return 'forward' if b > a else 'back' if b < a else 'same'


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def transitions_csv(text, by='region', min_words=6, max_gap=0, min_works=1, within=NONE,
                    min_steps=1, min_step_works=2, min_share=0):
    """The bytes `ao3.py transitions` writes for a match CSV's text: (transitions,
    transitions-units)."""
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

    def text_of(o):
        return label[o][0] if o in label else cr.UNKNOWN_WORD
    if by == 'region':
        cov = cr.coverage(recs, len(names), min_words, max_gap)
        unit_of, bounds = cr.regions_of(cov, n_script, min_works)
        about = [(a, b, label[a][1], label[a][2], ' '.join(text_of(o) for o in range(a, b + 1)))
                 for a, b in bounds]                 # a region starts at a record
    else:
        col = {'character': 1, 'scene': 2}[by]
        unit_of, found = cr.labels_of({o: lab[col] for o, lab in label.items()}, n_script)
        about = []
        for u, name in enumerate(found):
            at = [o for o in range(n_script) if unit_of[o] == u]
            about.append((min(at), max(at), name if col == 1 else '', name if col == 2 else '', ''))
    units, found = transitions(recs, len(names), n_script, unit_of, len(about), min_words,
                               max_gap, within, min_steps, min_step_works, min_share)
    total = sum(u['steps_out'] for u in units)
    ctab = [CELL_FIELDS]
    for c in sorted(found, key=lambda c: (-c['steps'], c['a'], c['b'])):
        a, b, n = c['a'], c['b'], c['steps']
        ctab.append([a + 1, b + 1] + list(about[a][:4]) + list(about[b][:4])
                    + [n, c['advances'], c['works'], share_percent(n, c['steps_out_a']),
                       lift_permille(n, total, c['steps_out_a'], c['steps_in_b']),
                       direction(a, b), names[c['first_work']], about[a][4], about[b][4]])
    utab = [UNIT_FIELDS]
    for u, v in enumerate(units):
        utab.append([u + 1] + list(about[u][:4])
                    + [v[k] for k in UNIT_KEYS[:8]]
                    + ['' if v['best_next'] == NONE else v['best_next'] + 1, v['best_steps'],
                       about[u][4]])
    return _csv(ctab), _csv(utab)
