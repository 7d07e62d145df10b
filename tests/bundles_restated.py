"""The `bundles` contract restated in plain Python on tests/companions_restated.py: a set of
works per unit, and the frequent sets of units mined level by level exactly as the contract
words it (F_k in lexicographic order, the candidates of level k + 1 joined from the pairs of
F_k that agree in their first k - 1 units).  The oracle of tests/test_bundles_host.py and
tests/test_gpu_bundles.py and of the committed tests/golden/bundles_*.csv.  The product never
imports it."""

from tests import companions_restated as cr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
MAX_SIZE = 8
MAX_SETS = 1 << 22
SET_FIELDS = ['SET', 'SIZE', 'UNITS', 'WORKS', 'LEAST_UNIT_WORKS', 'SHARE_PERCENT',
              'LIFT_PERMILLE', 'CLOSED', 'EXTENSIONS', 'FIRST_FAN_WORK_FILENAME',
              'FIRST_WORD_INDEXES', 'CHARACTERS', 'SCENES', 'TEXTS']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'SETS', 'LARGEST_SET', 'BEST_SET', 'TEXT']
LEVEL_FIELDS = ['SIZE', 'CANDIDATES', 'FREQUENT', 'CLOSED', 'MAXIMAL', 'PRINTED']
SET_KEYS = ['units', 'size', 'works', 'first_work', 'extensions', 'closed']
UNIT_KEYS = ['works', 'sets', 'largest']
LEVEL_KEYS = ['size', 'candidates', 'frequent', 'closed', 'maximal']


class TooManySets(NotImplementedError):
    """A level with more candidates than max_sets: .level and .count say which and how many."""

    def __init__(self, level, count):
        NotImplementedError.__init__(self, "level %d has %d candidate sets" % (level, count))
        self.level, self.count = level, count


def mine(members, min_all=5, max_size=4, max_sets=MAX_SETS):
    """members[u]: the set of works quoting unit u.  Returns (units, levels, sets): a dict of
    UNIT_KEYS per unit, a dict of LEVEL_KEYS per size 2 .. max_size + 1, a dict of SET_KEYS per
    frequent set of 2 .. max_size units, by size, then lexicographically."""
    if min_all < 1 or not 2 <= max_size <= MAX_SIZE:
        raise ValueError("min_all must be at least 1, max_size 2 to 8")
    n_units = len(members)
    single = [u for u in range(n_units) if len(members[u]) >= min_all]
    # F_2: the pairs companions keeps under both >= min_all
    level = []
    for a in range(n_units):
        for b in range(a + 1, n_units):
            both = members[a] & members[b]
            if len(both) >= min_all:
                level.append(((a, b), both))
    if len(level) > max_sets:
        raise TooManySets(2, len(level))
    by_size = {2: level}
    cands = {2: len(single) * (len(single) - 1) // 2}
    for k in range(2, max_size + 1):
        prev, joined = by_size[k], []
        for i in range(len(prev)):
            for j in range(i + 1, len(prev)):
                if prev[i][0][:-1] != prev[j][0][:-1]:
                    break                            # sorted: the group is contiguous
                joined.append((i, j))
        cands[k + 1] = len(joined)
        if len(joined) > max_sets:
            raise TooManySets(k + 1, len(joined))
        nxt = []
        for i, j in joined:                          # (i, j) order: lexicographic again
            works = prev[i][1] & members[prev[j][0][-1]]
            if len(works) >= min_all:
                nxt.append((prev[i][0] + (prev[j][0][-1],), works))
        assert [s for s, _ in nxt] == sorted(s for s, _ in nxt)
        by_size[k + 1] = nxt
    units = [dict(works=len(m), sets=0, largest=0) for m in members]
    levels, sets = [], []
    for k in range(2, max_size + 2):
        above = {}
        have = {s: len(works) for s, works in by_size[k]}
        if k <= max_size:
            for s, works in by_size[k + 1]:
                for out in range(k + 1):
                    sub = s[:out] + s[out + 1:]
                    n, same = above.get(sub, (0, False))
                    above[sub] = (n + 1, same or len(works) == have[sub])
        n_closed = n_max = 0
        for s, works in by_size[k] if k <= max_size else []:
            ext, same = above.get(s, (0, False))
            n_closed += not same
            n_max += ext == 0
            sets.append(dict(units=list(s) + [NONE] * (MAX_SIZE - k), size=k, works=len(works),
                             first_work=min(works), extensions=ext, closed=int(not same)))
            for u in s:
                units[u]['sets'] += 1
                units[u]['largest'] = max(units[u]['largest'], k)
        last = k > max_size
        levels.append(dict(size=k, candidates=cands[k], frequent=len(by_size[k]),
                           closed=NONE if last else n_closed, maximal=NONE if last else n_max))
    return units, levels, sets


def members_of(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0):
    """The set of works quoting each unit, under the checks of companions."""
    if min_words < 1:
        raise ValueError("min_words must be at least 1")
    if len(records) >= 1 << 32:
        raise NotImplementedError("too many records")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = cr.coverage(records, n_works, min_words, max_gap)
    members = [set() for _ in range(n_units)]
    for w, c in enumerate(cov):
        for o in c:
            if unit_of[o] != NONE:
                members[unit_of[o]].add(w)
    return members


def bundles(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0, min_all=5,
            max_size=4, max_sets=MAX_SETS):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).  mine() over the
    works quoting each unit."""
    if min_all < 1 or not 2 <= max_size <= MAX_SIZE:
        raise ValueError("min_all must be at least 1, max_size 2 to 8")
    return mine(members_of(records, n_works, n_script, unit_of, n_units, min_words, max_gap),
                min_all, max_size, max_sets)


def lift_permille(works, n_active, unit_works):
    den = 1
    for w in unit_works:
        den *= w
    return works * n_active ** (len(unit_works) - 1) * 1000 // den


def tables(units, levels, sets, about, names, n_active, by='region', max_size=4, every=False):
    """The three files' rows with their headers, from the records of mine()."""
    listed = sorted((s for s in sets if every or s['closed']),
                    key=lambda s: (-s['works'], -s['size'], s['units'][:s['size']]))
    stab, best, printed = [SET_FIELDS], {}, {}
    for row, s in enumerate(listed, 1):
        us = s['units'][:s['size']]
        ws = [units[u]['works'] for u in us]
        for u in us:
            best.setdefault(u, row)
        printed[s['size']] = printed.get(s['size'], 0) + 1
        stab.append([row, s['size'], ' '.join(str(u + 1) for u in us), s['works'], min(ws),
                     s['works'] * 100 // min(ws), lift_permille(s['works'], n_active, ws),
                     s['closed'], s['extensions'], names[s['first_work']],
                     ' '.join(str(about[u][0]) for u in us),
                     ' | '.join(about[u][2] for u in us), ' | '.join(about[u][3] for u in us),
                     ' | '.join(about[u][4] for u in us) if by == 'region' else ''])
    utab = [UNIT_FIELDS]
    for u, v in enumerate(units):
        utab.append([u + 1] + list(about[u][:4])
                    + [v['works'], v['sets'], v['largest'], best.get(u, ''), about[u][4]])
    ltab = [LEVEL_FIELDS]
    for v in levels:
        last = v['size'] > max_size
        ltab.append([v['size'], v['candidates'], v['frequent'], '' if last else v['closed'],
                     '' if last else v['maximal'], printed.get(v['size'], 0)])
    return stab, utab, ltab


def bundles_csv(text, by='region', min_words=6, max_gap=0, min_works=1, min_all=5, max_size=4,
                every=False):
    """The bytes `ao3.py bundles` writes for a match CSV's text: (bundles, bundles-units,
    bundles-levels)."""
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
    cov = cr.coverage(recs, len(names), min_words, max_gap)
    n_active = sum(1 for c in cov if c)

    def text_of(o):
        return label[o][0] if o in label else cr.UNKNOWN_WORD
    if by == 'region':
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
    units, levels, sets = bundles(recs, len(names), n_script, unit_of, len(about), min_words,
                                  max_gap, min_all, max_size)
    return tuple(cr._csv(t) for t in tables(units, levels, sets, about, names, n_active, by,
                                            max_size, every))
