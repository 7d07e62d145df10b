"""The `routes` contract restated in plain Python on tests/transitions_restated.py: a work's
unit-bearing passages collapsed as `retellings` collapses SCENE_SEQUENCE, a per-work dynamic
programme for support, and the frequent routes mined level by level exactly as the contract
words it (F_k in lexicographic order, the candidates of level k + 1 joined from the pairs of
F_k where one's last k - 1 units are the other's first).  The oracle of
tests/test_routes_host.py and tests/test_gpu_routes.py and of the committed
tests/golden/routes_*.csv.  The product never imports it."""

from tests import companions_restated as cr
from tests import passages_restated as pr
from tests import transitions_restated as tr

NONE = 0xFFFFFFFF
MAX_LENGTH = 8
MAX_SKIP = 63
MAX_SETS = 1 << 22
ROUTE_FIELDS = ['ROUTE', 'LENGTH', 'UNITS', 'WORKS', 'PREFIX_WORKS', 'CONTINUE_PERCENT',
                'DIRECTION', 'CLOSED', 'FORWARD', 'BACKWARD', 'FIRST_FAN_WORK_FILENAME',
                'FIRST_WORD_INDEXES', 'CHARACTERS', 'SCENES', 'TEXTS']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'ROUTES', 'LONGEST_ROUTE', 'BEST_ROUTE', 'TEXT']
LEVEL_FIELDS = ['LENGTH', 'CANDIDATES', 'FREQUENT', 'CLOSED', 'PRINTED']
ROUTE_KEYS = ['units', 'length', 'works', 'first_work', 'prefix_works', 'forward', 'backward',
              'closed']
UNIT_KEYS = ['works', 'routes', 'longest']
LEVEL_KEYS = ['length', 'candidates', 'frequent', 'closed']


class TooManyRoutes(NotImplementedError):
    """A level with more candidates than max_sets: .level and .count say which and how many."""

    def __init__(self, level, count):
        NotImplementedError.__init__(self, "level %d has %d candidate routes" % (level, count))
        self.level, self.count = level, count


def collapse(units):
    """Consecutive equal entries written once."""
    out = []
    for u in units:
        if not out or out[-1] != u:
            out.append(u)
    return out


def supports(seq, route, max_skip=NONE):
    """Whether there are p_1 < ... < p_k with seq[p_i] = route[i] and p_i+1 - p_i <=
    max_skip + 1: ends[p] says an occurrence of the route so far ends at p."""
    reach = len(seq) if max_skip == NONE else max_skip + 1
    ends = [s == route[0] for s in seq]
    for a in route[1:]:
        nxt, last = [False] * len(seq), None             # last: the closest end in front of p
        for p in range(len(seq)):
            nxt[p] = seq[p] == a and last is not None and p - last <= reach
            if ends[p]:
                last = p
        ends = nxt
    return any(ends)


def mine(seqs, n_units, max_skip=NONE, min_all=5, max_length=4, max_sets=MAX_SETS):
    """seqs: {work: its collapsed sequence}.  Returns (units, levels, routes): a dict of
    UNIT_KEYS per unit, a dict of LEVEL_KEYS per length 2 .. max_length + 1, a dict of
    ROUTE_KEYS per frequent route of 2 .. max_length units, by length, then
    lexicographically."""
    if min_all < 1 or not 2 <= max_length <= MAX_LENGTH:
        raise ValueError("min_all must be at least 1, max_length 2 to 8")
    if max_skip != NONE and not 0 <= max_skip <= MAX_SKIP:
        raise ValueError("max_skip must be 0 to 63, or none")
    seqs = {w: s for w, s in seqs.items() if len(s) >= 2}

    holding = {}
    for w, s in seqs.items():
        for u in set(s):
            holding.setdefault(u, set()).add(w)

    def works_of(route):
        among = set.intersection(*(holding.get(u, set()) for u in set(route)))
        return sorted(w for w in among if supports(seqs[w], route, max_skip))
    uworks = [len(holding.get(u, ())) for u in range(n_units)]
    by_len = {1: [((u,), None) for u in range(n_units) if uworks[u] >= min_all]}
    cands = {}
    for k in range(1, max_length + 1):
        prev, joined = by_len[k], []
        starting = {}
        for j, (q, _) in enumerate(prev):                # (the j of one start are contiguous)
            starting.setdefault(q[:-1], []).append(j)
        for i, (p, _) in enumerate(prev):
            joined += [(i, j) for j in starting.get(p[1:], []) if k > 1 or i != j]
        cands[k + 1] = len(joined)
        if len(joined) > max_sets:
            raise TooManyRoutes(k + 1, len(joined))
        nxt = []
        for i, j in joined:                              # (i, j) order: lexicographic again
            route = prev[i][0] + (prev[j][0][-1],)
            works = works_of(route)
            if len(works) >= min_all:
                nxt.append((route, works))
        assert [r for r, _ in nxt] == sorted(r for r, _ in nxt)
        by_len[k + 1] = nxt
    units = [dict(works=w, routes=0, longest=0) for w in uworks]
    levels, routes = [], []
    for k in range(2, max_length + 2):
        have = {r: len(works) for r, works in by_len[k]}
        below = dict(by_len[k - 1])
        fwd, bwd, same = {}, {}, set()
        if k <= max_length:
            for r, works in by_len[k + 1]:
                fwd[r[:-1]] = fwd.get(r[:-1], 0) + 1
                bwd[r[1:]] = bwd.get(r[1:], 0) + 1
                same |= {x for x in (r[:-1], r[1:]) if have[x] == len(works)}
        n_closed = 0
        for r, works in by_len[k] if k <= max_length else []:
            n_closed += r not in same
            routes.append(dict(units=list(r) + [NONE] * (MAX_LENGTH - k), length=k,
                               works=len(works), first_work=works[0],
                               prefix_works=uworks[r[0]] if k == 2 else len(below[r[:-1]]),
                               forward=fwd.get(r, 0), backward=bwd.get(r, 0),
                               closed=int(r not in same)))
            for u in set(r):                             # a unit that returns counts once
                units[u]['routes'] += 1
                units[u]['longest'] = max(units[u]['longest'], k)
        levels.append(dict(length=k, candidates=cands[k], frequent=len(by_len[k]),
                           closed=NONE if k > max_length else n_closed))
    return units, levels, routes


def sequences(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0):
    """{work: its collapsed sequence of units}, under the checks of transitions."""
    if min_words < 1:
        raise ValueError("min_words must be at least 1")
    if len(records) >= 1 << 32:
        raise NotImplementedError("too many records")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    per_work = {}
    for p in tr.sequence(records, unit_of, min_words, max_gap):
        per_work.setdefault(p['work'], []).append(p['unit'])
    return {w: collapse(us) for w, us in per_work.items()}


def routes(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0, max_skip=NONE,
           min_all=5, max_length=4, max_sets=MAX_SETS):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).  mine() over the
    works' collapsed sequences."""
    if min_all < 1 or not 2 <= max_length <= MAX_LENGTH:
        raise ValueError("min_all must be at least 1, max_length 2 to 8")
    if max_skip != NONE and not 0 <= max_skip <= MAX_SKIP:
        raise ValueError("max_skip must be 0 to 63, or none")
    if not records or not n_units:
        seqs = {}
    else:
        seqs = sequences(records, n_works, n_script, unit_of, n_units, min_words, max_gap)
    return mine(seqs, n_units, max_skip, min_all, max_length, max_sets)


def direction(units):
    if all(b > a for a, b in zip(units, units[1:])):
        return 'forward'
    if all(b < a for a, b in zip(units, units[1:])):
        return 'back'
    return 'mixed'


def tables(units, levels, found, about, names, by='region', max_length=4, every=False):
    """The three files' rows with their headers, from the records of mine()."""
    listed = sorted((r for r in found if every or r['closed']),
                    key=lambda r: (-r['works'], -r['length'], r['units'][:r['length']]))
    rtab, best, printed = [ROUTE_FIELDS], {}, {}
    for row, r in enumerate(listed, 1):
        us = r['units'][:r['length']]
        for u in us:
            best.setdefault(u, row)
        printed[r['length']] = printed.get(r['length'], 0) + 1
        rtab.append([row, r['length'], ' > '.join(str(u + 1) for u in us), r['works'],
                     r['prefix_works'], r['works'] * 100 // r['prefix_works'], direction(us),
                     r['closed'], r['forward'], r['backward'], names[r['first_work']],
                     ' '.join(str(about[u][0]) for u in us),
                     ' | '.join(about[u][2] for u in us), ' | '.join(about[u][3] for u in us),
                     ' | '.join(about[u][4] for u in us) if by == 'region' else ''])
    utab = [UNIT_FIELDS]
    for u, v in enumerate(units):
        utab.append([u + 1] + list(about[u][:4])
                    + [v['works'], v['routes'], v['longest'], best.get(u, ''), about[u][4]])
    ltab = [LEVEL_FIELDS]
    for v in levels:
        ltab.append([v['length'], v['candidates'], v['frequent'],
                     '' if v['length'] > max_length else v['closed'],
                     printed.get(v['length'], 0)])
    return rtab, utab, ltab


def routes_csv(text, by='region', min_words=6, max_gap=0, min_works=1, min_all=5, max_length=4,
               max_skip=NONE, every=False):
    """The bytes `ao3.py routes` writes for a match CSV's text: (routes, routes-units,
    routes-levels)."""
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
    units, levels, found = routes(recs, len(names), n_script, unit_of, len(about), min_words,
                                  max_gap, max_skip, min_all, max_length)
    return tuple(cr._csv(t) for t in tables(units, levels, found, about, names, by, max_length,
                                            every))
