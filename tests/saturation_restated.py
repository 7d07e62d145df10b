"""The `saturation` contract restated in plain Python from its definitions: the oracle of the
tests (tests/test_saturation_host.py, tests/test_gpu_saturation.py) and of the committed
tests/golden/saturation_*.csv.  The product never imports it.

Python integers for the hash, sets for coverage and units (tests/companions_restated.py),
sorted() for the order statistics, the values below every threshold counted in a sorted list
for the curve: no bit rows, no buckets, no histograms, no scans.  hash_np is the same hash over numpy arrays, for the
tests that need many of them; tests/test_saturation_host.py holds it to the plain form."""

import bisect
import csv
import io

import numpy as np

from tests import companions_restated as cr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
MASK = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
POINT_FIELDS = ['POINT', 'SAMPLE_PPM', 'WORKS_LOW', 'WORKS_MEDIAN', 'WORKS_HIGH',
                'WORKS_MEAN_MILLI', 'UNITS_LOW', 'UNITS_MEDIAN', 'UNITS_HIGH', 'UNITS_MIN',
                'UNITS_MAX', 'UNITS_MEAN_MILLI', 'UNITS_PERCENT', 'NEW_PER_WORK_MILLI']
PERMUTATION_FIELDS = ['PERMUTATION', 'HALF_AT_PPM', 'NINETY_AT_PPM', 'ALL_AT_PPM']
SUMMARY_FIELDS = ['WORKS', 'ACTIVE_WORKS', 'UNITS', 'UNITS_QUOTED', 'QUOTED_BY_ONE',
                  'QUOTED_BY_TWO', 'UNSEEN_ESTIMATE', 'ESTIMATED_TOTAL', 'SEEN_PERCENT',
                  'HALF_AT_PPM', 'NINETY_AT_PPM', 'ALL_AT_PPM']
POINT_KEYS = ['units_low', 'units_median', 'units_high', 'units_min', 'units_max', 'works_low',
              'works_median', 'works_high', 'units_sum', 'works_sum']
PERM_KEYS = ['half_at', 'ninety_at', 'all_at']
SUMMARY_KEYS = ['n_active', 'units_quoted', 'singletons', 'doubletons']
UNKNOWN_WORD = '[?]'


def hash32(seed, r, w):
    z = (((r << 32) | w) + seed * GOLDEN_GAMMA) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z = z ^ (z >> 31)
    return z >> 32


def hash_np(seed, rs, ws):
    """hash32 over every (r, w) of the two integer arrays: an int64 array [len(rs)][len(ws)]."""
    rs = np.asarray(rs, dtype=np.uint64).reshape(-1, 1)
    ws = np.asarray(ws, dtype=np.uint64).reshape(1, -1)
    with np.errstate(over='ignore'):
        z = ((rs << np.uint64(32)) | ws) + np.uint64((seed * GOLDEN_GAMMA) & MASK)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.int64)


def threshold(c, points):
    """T_c."""
    return c * (1 << 32) // points


def bucket(h, points):
    """The first point whose sample holds a time h, as the issue's formula has it."""
    return ((h + 1) * points + (1 << 32) - 1) >> 32


def bucket_by_definition(h, points):
    return next(c for c in range(1, points + 1) if h < threshold(c, points))


def cut(permutations, level):
    return permutations * (100 - level) // 200


def unseen_estimate(n_works, q1, q2):
    return ((n_works - 1) * q1 * (q1 - 1)) // (n_works * 2 * (q2 + 1)) if n_works else 0


def saturation(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0,
               permutations=1000, points=100, seed=0, level=95, fast=False):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).  Returns (works,
    one dict of POINT_KEYS per point, one dict of PERM_KEYS per order, a dict of SUMMARY_KEYS,
    first[u][r]).  `fast`: the hashes from hash_np."""
    if min_words < 1 or not 1 <= permutations <= 4096 or not 50 <= level <= 99:
        raise ValueError("min_words at least 1, permutations 1 to 4096, level 50 to 99")
    if not 1 <= points <= 1024:
        raise ValueError("points 1 to 1024")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed outside 64 bits")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for rec in records:
        if rec[0] >= n_works or rec[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = cr.coverage(records, n_works, min_words, max_gap)
    active = [w for w in range(n_works) if cov[w]]
    members = [set() for _ in range(n_units)]
    for w, c in enumerate(cov):
        for o in c:
            if unit_of[o] != NONE:
                members[unit_of[o]].add(w)
    R, K = permutations, points
    if fast:
        h = hash_np(seed, range(R), range(n_works)).tolist()
    else:
        h = [[hash32(seed, r, w) for w in range(n_works)] for r in range(R)]
    works = [len(s) for s in members]
    quoted = [u for u in range(n_units) if works[u] > 0]
    Q = len(quoted)
    first = [[min(h[r][w] for w in members[u]) if members[u] else NONE for r in range(R)]
             for u in range(n_units)]
    T = [threshold(c, K) for c in range(K + 1)]

    def below(values):
        """How many of the values lie below T_c, for c = 0..K."""
        s = sorted(values)
        return [bisect.bisect_left(s, T[c]) for c in range(K + 1)]
    n = [below(h[r][:n_works]) for r in range(R)]
    S = [below([first[u][r] for u in quoted]) for r in range(R)]
    t = cut(R, level)
    pts = []
    for c in range(1, K + 1):
        s = sorted(S[r][c] for r in range(R))
        m = sorted(n[r][c] for r in range(R))
        pts.append(dict(units_low=s[t], units_median=s[(R - 1) // 2], units_high=s[R - 1 - t],
                        units_min=s[0], units_max=s[R - 1], works_low=m[t],
                        works_median=m[(R - 1) // 2], works_high=m[R - 1 - t], units_sum=sum(s),
                        works_sum=sum(m)))
    perms = []
    for r in range(R):
        perms.append(dict(
            half_at=next(c for c in range(1, K + 1) if 2 * S[r][c] >= Q),
            ninety_at=next(c for c in range(1, K + 1) if 10 * S[r][c] >= 9 * Q),
            all_at=next(c for c in range(1, K + 1) if S[r][c] == Q)))
    summary = dict(n_active=len(active), units_quoted=Q,
                   singletons=sum(1 for x in works if x == 1),
                   doubletons=sum(1 for x in works if x == 2))
    return works, pts, perms, summary, first


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def saturation_csv(text, by='word', min_words=6, max_gap=0, min_works=1, permutations=1000,
                   points=100, seed=0, level=95):
    """The bytes `ao3.py saturation` writes for a match CSV's text: (saturation,
    saturation-permutations, saturation-summary)."""
    if min_works < 1 or max_gap < 0:
        raise ValueError("min_works at least 1, max_gap at least 0")
    rows = pr.read_rows(text)
    work_of, keyed = {}, []
    for k, r in enumerate(rows):
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
    keyed.sort(key=lambda x: (x[0], x[1]))           # stable: ties keep file order
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
        return _csv([POINT_FIELDS]), _csv([PERMUTATION_FIELDS]), _csv([SUMMARY_FIELDS])
    n_script = max(label) + 1
    cov = cr.coverage(recs, len(names), min_words, max_gap)
    if by == 'region':
        unit_of, bounds = cr.regions_of(cov, n_script, min_works)
        n_units = len(bounds)
    elif by == 'word':
        region_of, _ = cr.regions_of(cov, n_script, min_works)
        at = [o for o in range(n_script) if region_of[o] != NONE]
        unit_of = [NONE] * n_script
        for u, o in enumerate(at):
            unit_of[o] = u
        n_units = len(at)
    else:
        col = {'character': 1, 'scene': 2}[by]
        unit_of, found = cr.labels_of({o: lab[col] for o, lab in label.items()}, n_script)
        n_units = len(found)
    _, pts, perms, summary, _ = saturation(recs, len(names), n_script, unit_of, n_units,
                                           min_words, max_gap, permutations, points, seed, level)
    R, K, N = permutations, points, len(names)
    Q, q1, q2 = summary['units_quoted'], summary['singletons'], summary['doubletons']
    ptab, before = [POINT_FIELDS], dict(units_sum=0, works_sum=0)
    for c, p in enumerate(pts, 1):
        ptab.append([c, c * 1000000 // K, p['works_low'], p['works_median'], p['works_high'],
                     p['works_sum'] * 1000 // R, p['units_low'], p['units_median'],
                     p['units_high'], p['units_min'], p['units_max'], p['units_sum'] * 1000 // R,
                     p['units_median'] * 100 // max(1, Q),
                     (p['units_sum'] - before['units_sum']) * 1000
                     // max(1, p['works_sum'] - before['works_sum'])])
        before = p
    rtab = [PERMUTATION_FIELDS]
    for r, v in enumerate(perms):
        rtab.append([r + 1] + [v[k] * 1000000 // K for k in PERM_KEYS])
    unseen = unseen_estimate(N, q1, q2)
    stab = [SUMMARY_FIELDS,
            [N, summary['n_active'], n_units, Q, q1, q2, unseen, Q + unseen,
             Q * 100 // max(1, Q + unseen)]
            + [sorted(v[k] for v in perms)[(R - 1) // 2] * 1000000 // K for k in PERM_KEYS]]
    return _csv(ptab), _csv(rtab), _csv(stab)
