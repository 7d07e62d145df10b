"""The `trends` contract restated in plain Python from its definitions: the oracle of the tests
(tests/test_trends_host.py, tests/test_gpu_trends.py) and of the committed
tests/golden/trends_lines.*.csv.  The product never imports it.

Python integers for the hash (tests/intervals_restated.py), a list for the pool, sets for the
works quoting a unit (tests/contrast_restated.py), math.isqrt for the denominators: no bit rows,
no byte planes, no tiles.  `fast` takes the draw from numpy (contrast_restated.keys_np) for the
tests with a million works; tests/test_trends_host.py holds it to the plain form."""

import csv
import io
import math

import numpy as np

from tests import companions_restated as cr
from tests import contrast_restated as cn
from tests import groups_restated as gr
from tests import intervals_restated as ir
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
OUT = 0xFFFF
MAX_SPAN = 1024
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE',
               'QUOTING_WORKS', 'FIRST_PERIOD', 'LAST_PERIOD', 'MEAN_PERIOD_MILLI',
               'POOL_MEAN_PERIOD_MILLI', 'SHIFT_MILLI', 'DIRECTION', 'STATISTIC', 'GE', 'P_PPM',
               'ADJ_GE', 'ADJ_PPM', 'TEXT']
PERIOD_FIELDS = ['PERIOD', 'OFFSET', 'WORKS', 'ACTIVE_WORKS']
PERMUTATION_FIELDS = ['PERMUTATION', 'POOL_OFFSET_SUM', 'MAX_STATISTIC', 'MAX_UNIT']
UNIT_KEYS = ['quoting', 'ge', 'adj_ge', 'first_x', 'last_x', 'offset_sum', 'statistic', 'd']
PERM_KEYS = ['max_statistic', 'offset_sum', 'max_unit']
UNKNOWN_DATE, NO_METADATA = '(unknown date)', '(no metadata)'
UNKNOWN_WORD = '[?]'


def den(t, n):
    return math.isqrt((t * (n - t)) << 20)


def statistic(d, dn):
    return (abs(d) << 10) // dn if dn else 0


def draw(seed, r, w, n):
    """v: the pool position whose date work w takes in re-dating r."""
    return (ir.hash32(seed, r, w) * n) >> 32


def redated(when, permutations, seed, fast=False):
    """x_r(w) for every r, a list over the works (0 for a work outside the pool)."""
    pool = [w for w, x in enumerate(when) if x != OUT]
    n = len(pool)
    if fast:
        at, xs = np.array(pool, dtype=np.uint64), np.array([when[w] for w in pool], np.int64)
        out = []
        for r in range(permutations):
            row = np.zeros(len(when), dtype=np.int64)
            if n:
                v = (cn.keys_np(seed, r, at, 32) * np.uint64(n)) >> np.uint64(32)
                row[at.astype(np.int64)] = xs[v.astype(np.int64)]
            out.append(row.tolist())
        return out
    out = []
    for r in range(permutations):
        row = [0] * len(when)
        for w in pool:
            row[w] = when[pool[draw(seed, r, w, n)]]
        out.append(row)
    return out


def trends(records, n_works, n_script, unit_of, n_units, when, min_words=6, max_gap=0,
           min_quoting=5, permutations=1000, seed=0, fast=False):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix); when: n_works
    values, x(w) below 1024 or 0xFFFF (outside the pool).  Returns (one dict of UNIT_KEYS per
    unit, one dict of PERM_KEYS per re-dating, s_r(u) as [n_units][permutations])."""
    if min_words < 1 or min_quoting < 1 or not 1 <= permutations <= 4096:
        raise ValueError("min_words and min_quoting at least 1, permutations 1 to 4096")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed inside 64 bits")
    if n_works > 1 << 20:
        raise NotImplementedError("too many works")
    if len(when) != n_works or any(x != OUT and not 0 <= x < MAX_SPAN for x in when):
        raise ValueError("an offset per work, below 1024 or 0xFFFF")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    active, members = cn.quoting(records, n_works, n_script, unit_of, n_units, min_words, max_gap)
    pool = [w for w in range(n_works) if when[w] != OUT]
    n, P = len(pool), permutations
    big_x = sum(when[w] for w in pool)
    quoters = [sorted(w for w in m if when[w] != OUT) for m in members]
    t = [len(q) for q in quoters]
    s = [sum(when[w] for w in q) for q in quoters]
    d = [s[u] * n - t[u] * big_x for u in range(n_units)]
    dn = [den(t[u], n) for u in range(n_units)]
    x_r = redated(when, P, seed, fast)
    big_x_r = [sum(row) for row in x_r]
    s_r = [[sum(x_r[r][w] for w in q) for r in range(P)] for q in quoters]
    d_r = [[s_r[u][r] * n - t[u] * big_x_r[r] for r in range(P)] for u in range(n_units)]
    family = [u for u in range(n_units) if t[u] >= min_quoting and t[u] < n]
    perms = []
    for r in range(P):
        zs = [statistic(d_r[u][r], dn[u]) for u in family]
        mx = max(zs, default=0)
        perms.append(dict(max_statistic=mx, offset_sum=big_x_r[r],
                          max_unit=family[zs.index(mx)] if family else NONE))
    units = []
    for u in range(n_units):
        z = statistic(d[u], dn[u])
        units.append(dict(
            quoting=t[u], ge=sum(1 for r in range(P) if abs(d_r[u][r]) >= abs(d[u])),
            adj_ge=sum(1 for p in perms if p['max_statistic'] >= z) if u in family else NONE,
            first_x=min((when[w] for w in quoters[u]), default=NONE),
            last_x=max((when[w] for w in quoters[u]), default=NONE),
            offset_sum=s[u], statistic=z, d=d[u]))
    return units, perms, s_r


# ---- the periods -------------------------------------------------------------------------

def number_of(key):
    """A key YYYY has the number YYYY, a key YYYY-MM the number YYYY * 12 + MM - 1."""
    return int(key) if len(key) == 4 else int(key[:4]) * 12 + int(key[5:7]) - 1


def label_of(number, by):
    return '%04d' % number if by == 'year' else '%04d-%02d' % (number // 12, number % 12 + 1)


def periods_of(names, meta, by):
    """(when per work, base, the key of every work) of the works `names` under the metadata rows
    `meta` ({stem: row})."""
    if by not in ('year', 'month'):
        raise ValueError("--by takes year or month")
    keys = []
    for name in names:
        s = gr.stem(name)
        keys.append(gr.keys_of(meta[s], by)[0] if s in meta else NO_METADATA)
    numbers = [None if k in (UNKNOWN_DATE, NO_METADATA) else number_of(k) for k in keys]
    dated = [x for x in numbers if x is not None]
    if not dated:
        raise ValueError("an empty pool")
    base = min(dated)
    if max(dated) == base:
        raise ValueError("a pool of one period")
    if max(dated) - base >= MAX_SPAN:
        raise ValueError("a span above 1023")
    return [OUT if x is None else x - base for x in numbers], base, keys


# ---- the command -------------------------------------------------------------------------

def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def trends_csv(text, meta_text, by='year', unit='region', min_words=6, max_gap=0, min_works=1,
               min_quoting=5, permutations=1000, seed=0):
    """The bytes `ao3.py trends` writes for a match CSV's and a metadata CSV's text:
    (trends, trends-periods, trends-permutations)."""
    if min_works < 1 or max_gap < 0:
        raise ValueError("min_works at least 1, max_gap at least 0")
    if by not in ('year', 'month'):
        raise ValueError("--by takes year or month")
    meta = gr.read_meta(meta_text, by)
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
    if not rows:
        return _csv([UNIT_FIELDS]), _csv([PERIOD_FIELDS]), _csv([PERMUTATION_FIELDS])
    when, base, keys = periods_of(names, meta, by)
    n_script = max(label) + 1
    cov = cr.coverage(recs, len(names), min_words, max_gap)

    def text_of(o):
        return label[o][0] if o in label else UNKNOWN_WORD
    if unit == 'region':
        unit_of, bounds = cr.regions_of(cov, n_script, min_works)
        about = [(a, b, label[a][1], label[a][2], ' '.join(text_of(o) for o in range(a, b + 1)))
                 for a, b in bounds]
    elif unit == 'word':
        region_of, _ = cr.regions_of(cov, n_script, min_works)
        at = [o for o in range(n_script) if region_of[o] != NONE]
        unit_of = [NONE] * n_script
        for u, o in enumerate(at):
            unit_of[o] = u
        about = [(o, o) + (label[o][1:] if o in label else ('', '')) + (text_of(o),) for o in at]
    else:
        col = {'character': 1, 'scene': 2}[unit]
        unit_of, found = cr.labels_of({o: lab[col] for o, lab in label.items()}, n_script)
        about = []
        for u, name in enumerate(found):
            at = [o for o in range(n_script) if unit_of[o] == u]
            about.append((min(at), max(at), name if col == 1 else '', name if col == 2 else '', ''))
    units, perms, _ = trends(recs, len(names), n_script, unit_of, len(about), when, min_words,
                             max_gap, min_quoting, permutations, seed)
    pool = [x for x in when if x != OUT]
    n, big_x, P = len(pool), sum(pool), permutations
    family = [u for u, v in enumerate(units) if v['adj_ge'] != NONE]
    family.sort(key=lambda u: (units[u]['adj_ge'], -units[u]['statistic'], u))
    utab = [UNIT_FIELDS]
    for u in family:
        v = units[u]
        t, s = v['quoting'], v['offset_sum']
        utab.append([u + 1] + list(about[u][:4])
                    + [t, label_of(base + v['first_x'], by), label_of(base + v['last_x'], by),
                       base * 1000 + s * 1000 // t, base * 1000 + big_x * 1000 // n,
                       abs(v['d']) * 1000 // (t * n),
                       'later' if v['d'] > 0 else 'earlier' if v['d'] < 0 else '=',
                       v['statistic'], v['ge'], (v['ge'] + 1) * 1000000 // (P + 1), v['adj_ge'],
                       (v['adj_ge'] + 1) * 1000000 // (P + 1), about[u][4]])
    active = [bool(c) for c in cov]
    dtab = [PERIOD_FIELDS]
    for x in range(max(pool) + 1):
        mine = [w for w in range(len(names)) if when[w] == x]
        dtab.append([label_of(base + x, by), x, len(mine), sum(1 for w in mine if active[w])])
    for key in (UNKNOWN_DATE, NO_METADATA):
        mine = [w for w in range(len(names)) if keys[w] == key]
        dtab.append([key, '', len(mine), sum(1 for w in mine if active[w])])
    ptab = [PERMUTATION_FIELDS]
    for r, p in enumerate(perms):
        ptab.append([r + 1, p['offset_sum'], p['max_statistic'],
                     '' if p['max_unit'] == NONE else p['max_unit'] + 1])
    return _csv(utab), _csv(dtab), _csv(ptab)
