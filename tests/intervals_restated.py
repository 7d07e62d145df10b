"""The `intervals` contract restated in plain Python from its definitions: the oracle of the
tests (tests/test_intervals_host.py, tests/test_gpu_intervals.py) and of the committed
tests/golden/intervals_*.csv.  The product never imports it.

Python integers for the hash and the table, sets for coverage and units
(tests/companions_restated.py), sorted() for the order statistics: no bit rows, no bytes, no
tiles.  mult_np is the same multiplicity over numpy arrays, for the tests that need many of
them; tests/test_intervals_host.py holds it to the plain form."""

import csv
import decimal
import io

import numpy as np

from tests import companions_restated as cr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
MASK = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
T = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777,
     4294923276, 4294962463, 4294966817, 4294967252, 4294967292, 4294967295)
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'WORKS_LOW', 'WORKS_MEDIAN', 'WORKS_HIGH', 'PPM', 'PPM_LOW', 'PPM_MEDIAN',
               'PPM_HIGH', 'MEAN_MILLI', 'RANK', 'NEXT', 'AHEAD_OF_NEXT', 'TIED_WITH_NEXT',
               'BEHIND_NEXT', 'TEXT']
REPLICATE_FIELDS = ['REPLICATE', 'RESAMPLED_WORKS', 'RESAMPLED_ACTIVE', 'UNITS_QUOTED']
UNIT_KEYS = ['works', 'works_low', 'works_median', 'works_high', 'ppm', 'ppm_low', 'ppm_median',
             'ppm_high', 'rank', 'next', 'ahead', 'tied', 'behind', 'mean_milli']
REPLICATE_KEYS = ['resampled_works', 'resampled_active', 'units_quoted']
UNKNOWN_WORD = '[?]'


def poisson_table(digits=80):
    """floor(2^32 * sum_{i <= k} e^-1 / i!) for k = 0..12, in decimals of `digits` digits."""
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        e_inv = 1 / decimal.Decimal(1).exp()
        out, term, cdf = [], e_inv, decimal.Decimal(0)
        for k in range(13):
            if k:
                term = term / k
            cdf += term
            out.append(int((cdf * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
        return tuple(out)


def hash32(seed, b, w):
    z = (((b << 32) | w) + seed * GOLDEN_GAMMA) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z = z ^ (z >> 31)
    return z >> 32


def mult(seed, b, w):
    h = hash32(seed, b, w)
    return sum(1 for t in T if h >= t)


def mult_np(seed, bs, ws):
    """mult over every (b, w) of the two integer arrays: a uint8 array [len(bs)][len(ws)]."""
    bs = np.asarray(bs, dtype=np.uint64).reshape(-1, 1)
    ws = np.asarray(ws, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over='ignore'):
        z = ((bs << np.uint64(32)) | ws) + np.uint64((seed * GOLDEN_GAMMA) & MASK)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    h = z >> np.uint64(32)
    out = np.zeros(h.shape, dtype=np.uint8)
    for t in T:
        out += h >= np.uint64(t)
    return out


def cut(replicates, level):
    return replicates * (100 - level) // 200


def order_stats(values, level):
    """(LOW, MEDIAN, HIGH) of the B values."""
    s = sorted(values)
    n = len(s)
    t = cut(n, level)
    return s[t], s[(n - 1) // 2], s[n - 1 - t]


def observed_order(works):
    """The units by works descending, then unit ascending."""
    return sorted(range(len(works)), key=lambda u: (-works[u], u))


def intervals(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0,
              replicates=1000, seed=0, level=95, fast=False):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).  Returns (one dict
    of UNIT_KEYS per unit, one dict of REPLICATE_KEYS per replicate).  `fast`: the multiplicities
    from mult_np."""
    if min_words < 1 or not 1 <= replicates <= 4096 or not 50 <= level <= 99:
        raise ValueError("min_words at least 1, replicates 1 to 4096, level 50 to 99")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed outside 64 bits")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = cr.coverage(records, n_works, min_words, max_gap)
    active = [w for w in range(n_works) if cov[w]]
    members = [set() for _ in range(n_units)]
    for w, c in enumerate(cov):
        for o in c:
            if unit_of[o] != NONE:
                members[unit_of[o]].add(w)
    B = replicates
    if fast:
        m = mult_np(seed, range(B), range(n_works)).astype(np.int64).tolist()
    else:
        m = [[mult(seed, b, w) for w in range(n_works)] for b in range(B)]
    N = [sum(m[b]) for b in range(B)]
    A = [sum(m[b][w] for w in active) for b in range(B)]
    c = [[sum(m[b][w] for w in members[u]) for b in range(B)] for u in range(n_units)]
    works = [len(s) for s in members]
    order = observed_order(works)
    nxt = [NONE] * n_units
    for at, u in enumerate(order[:-1]):
        nxt[u] = order[at + 1]
    units = []
    for u in range(n_units):
        low, med, high = order_stats(c[u], level)
        plow, pmed, phigh = order_stats([c[u][b] * 1000000 // max(1, N[b]) for b in range(B)],
                                        level)
        v = nxt[u]
        against = [0, 0, 0] if v == NONE else \
            [sum(1 for b in range(B) if c[u][b] > c[v][b]),
             sum(1 for b in range(B) if c[u][b] == c[v][b]),
             sum(1 for b in range(B) if c[u][b] < c[v][b])]
        units.append(dict(works=works[u], works_low=low, works_median=med, works_high=high,
                          ppm=works[u] * 1000000 // max(1, n_works), ppm_low=plow,
                          ppm_median=pmed, ppm_high=phigh,
                          rank=1 + sum(1 for x in works if x > works[u]), next=v,
                          ahead=against[0], tied=against[1], behind=against[2],
                          mean_milli=sum(c[u]) * 1000 // B))
    reps = [dict(resampled_works=N[b], resampled_active=A[b],
                 units_quoted=sum(1 for u in range(n_units) if c[u][b] > 0)) for b in range(B)]
    return units, reps


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def intervals_csv(text, by='region', min_words=6, max_gap=0, min_works=1, replicates=1000,
                  seed=0, level=95):
    """The bytes `ao3.py intervals` writes for a match CSV's text: (intervals,
    intervals-replicates)."""
    if min_works < 1 or max_gap < 0:
        raise ValueError("min_works at least 1, max_gap at least 0")
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
        return _csv([UNIT_FIELDS]), _csv([REPLICATE_FIELDS])
    n_script = max(label) + 1
    cov = cr.coverage(recs, len(names), min_words, max_gap)

    def text_of(o):
        return label[o][0] if o in label else UNKNOWN_WORD
    if by == 'region':
        unit_of, bounds = cr.regions_of(cov, n_script, min_works)
        about = [(a, b, label[a][1], label[a][2], ' '.join(text_of(o) for o in range(a, b + 1)))
                 for a, b in bounds]                 # a region starts at a record
    elif by == 'word':
        region_of, _ = cr.regions_of(cov, n_script, min_works)
        at = [o for o in range(n_script) if region_of[o] != NONE]
        unit_of = [NONE] * n_script
        for u, o in enumerate(at):
            unit_of[o] = u
        about = [(o, o) + (label[o][1:] if o in label else ('', '')) + (text_of(o),) for o in at]
    else:
        col = {'character': 1, 'scene': 2}[by]
        unit_of, found = cr.labels_of({o: lab[col] for o, lab in label.items()}, n_script)
        about = []
        for u, name in enumerate(found):
            at = [o for o in range(n_script) if unit_of[o] == u]
            about.append((min(at), max(at), name if col == 1 else '', name if col == 2 else '', ''))
    units, reps = intervals(recs, len(names), n_script, unit_of, len(about), min_words, max_gap,
                            replicates, seed, level)
    utab = [UNIT_FIELDS]
    for u, v in enumerate(units):
        against = ['', '', '', ''] if v['next'] == NONE else \
            [v['next'] + 1, v['ahead'], v['tied'], v['behind']]
        utab.append([u + 1] + list(about[u][:4])
                    + [v[k] for k in ('works', 'works_low', 'works_median', 'works_high', 'ppm',
                                      'ppm_low', 'ppm_median', 'ppm_high', 'mean_milli', 'rank')]
                    + against + [about[u][4]])
    rtab = [REPLICATE_FIELDS]
    for b, r in enumerate(reps):
        rtab.append([b + 1, r['resampled_works'], r['resampled_active'], r['units_quoted']])
    return _csv(utab), _csv(rtab)
