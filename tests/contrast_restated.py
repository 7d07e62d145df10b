"""The `contrast` contract restated in plain Python from its definitions: the oracle of the tests
(tests/test_contrast_host.py, tests/test_gpu_contrast.py) and of the committed
tests/golden/contrast_*.csv.  The product never imports it.

Python integers for the hash (tests/intervals_restated.py), sorted() on (key, w) for the
selection, sets for the counts, math.isqrt for the denominators: no bit rows, no tiles, no
radix passes."""

import csv
import io
import math

import numpy as np

from tests import companions_restated as cr
from tests import groups_restated as gr
from tests import intervals_restated as ir
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'A_WORKS',
               'B_WORKS', 'A_PPM', 'B_PPM', 'EXPECTED_A_MILLI', 'DIRECTION', 'RATIO_PERMILLE',
               'STATISTIC', 'GE', 'P_PPM', 'ADJ_GE', 'ADJ_PPM', 'TEXT']
SIDE_FIELDS = ['SIDE', 'KEYS', 'WORKS', 'ACTIVE_WORKS', 'UNITS_QUOTED']
PERMUTATION_FIELDS = ['PERMUTATION', 'A_ACTIVE_WORKS', 'MAX_STATISTIC', 'MAX_UNIT']
UNIT_KEYS = ['a_works', 'b_works', 'ge', 'adj_ge', 'statistic', 'd']
PERM_KEYS = ['max_statistic', 'a_active', 'max_unit']
EVERY_OTHER = '(every other work)'
UNKNOWN_WORD = '[?]'


def key(seed, r, w, key_bits):
    return ir.hash32(seed, r, w) >> (32 - key_bits) if key_bits else 0


def den(t, n):
    return math.isqrt((t * (n - t)) << 20)


def statistic(d, dn):
    return (abs(d) << 20) // dn if dn else 0


def keys_np(seed, r, ws, key_bits):
    """key over the integer array ws, for the tests with a million works;
    tests/test_contrast_host.py holds it to the plain form."""
    ws = np.asarray(ws, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = ((np.uint64(r) << np.uint64(32)) | ws) + np.uint64((seed * ir.GOLDEN_GAMMA) & ir.MASK)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(64 - key_bits)) if key_bits else np.zeros(len(ws), dtype=np.uint64)


def drawn(side, permutations, seed, key_bits, fast=False):
    """The side A of every permutation, a set of work numbers.  `fast`: the keys from
    keys_np, the order from a stable sort of them over the pool in work order."""
    pool = [w for w, s in enumerate(side) if s]
    na = sum(1 for w in pool if side[w] == 1)
    if fast:
        at = np.array(pool, dtype=np.int64)
        return [set(at[np.argsort(keys_np(seed, r, at, key_bits), kind='stable')[:na]].tolist())
                for r in range(permutations)]
    return [set(sorted(pool, key=lambda w: (key(seed, r, w, key_bits), w))[:na])
            for r in range(permutations)]


def quoting(records, n_works, n_script, unit_of, n_units, min_words, max_gap):
    """(the active works, the set of works quoting each unit)."""
    cov = cr.coverage(records, n_works, min_words, max_gap)
    members = [set() for _ in range(n_units)]
    for w, c in enumerate(cov):
        for o in c:
            if unit_of[o] != NONE:
                members[unit_of[o]].add(w)
    return {w for w in range(n_works) if cov[w]}, members


def contrast(records, n_works, n_script, unit_of, n_units, side, min_words=6, max_gap=0,
             min_quoting=5, permutations=1000, seed=0, key_bits=32, fast=False):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix); side: n_works
    values 0 (out), 1 (A), 2 (B).  Returns (one dict of UNIT_KEYS per unit, one dict of
    PERM_KEYS per permutation, a_r(u) as [n_units][permutations]).  `fast`: drawn's."""
    if min_words < 1 or min_quoting < 1 or not 1 <= permutations <= 4096:
        raise ValueError("min_words and min_quoting at least 1, permutations 1 to 4096")
    if not 0 <= key_bits <= 32 or not 0 <= seed < 1 << 64:
        raise ValueError("key_bits 0 to 32, seed inside 64 bits")
    if n_works > 1 << 20:
        raise NotImplementedError("too many works")
    if len(side) != n_works or any(s not in (0, 1, 2) for s in side):
        raise ValueError("a side byte per work, 0, 1 or 2")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    active, members = quoting(records, n_works, n_script, unit_of, n_units, min_words, max_gap)
    in_a = {w for w in range(n_works) if side[w] == 1}
    pool = {w for w in range(n_works) if side[w]}
    na, n = len(in_a), len(pool)
    sets = drawn(side, permutations, seed, key_bits, fast)
    P = permutations
    a = [len(m & in_a) for m in members]
    t = [len(m & pool) for m in members]
    dn = [den(t[u], n) for u in range(n_units)]
    d = [a[u] * n - t[u] * na for u in range(n_units)]
    a_r = [[len(m & sets[r]) for r in range(P)] for m in members]
    d_r = [[a_r[u][r] * n - t[u] * na for r in range(P)] for u in range(n_units)]
    family = [u for u in range(n_units) if t[u] >= min_quoting]
    perms = []
    for r in range(P):
        xs = [statistic(d_r[u][r], dn[u]) for u in family]
        mx = max(xs, default=0)
        perms.append(dict(max_statistic=mx, a_active=len(sets[r] & active),
                          max_unit=family[xs.index(mx)] if family else NONE))
    units = []
    for u in range(n_units):
        x = statistic(d[u], dn[u])
        units.append(dict(
            a_works=a[u], b_works=t[u] - a[u],
            ge=sum(1 for r in range(P) if abs(d_r[u][r]) >= abs(d[u])),
            adj_ge=sum(1 for p in perms if p['max_statistic'] >= x) if u in family else NONE,
            statistic=x, d=d[u]))
    return units, perms, a_r


# ---- the sides ---------------------------------------------------------------------------

def sides_of(names, meta, by, a_keys, b_keys):
    """(side bytes, (NA, NB, BOTH, OUT)) of the works `names` under the metadata rows `meta`
    ({stem: row}); b_keys empty: side B is every work that does not match A."""
    side, both, out = [], 0, 0
    for name in names:
        s = gr.stem(name)
        keys = gr.keys_of(meta[s], by) if s in meta else ['(no metadata)']
        is_a = any(k in a_keys for k in keys)
        is_b = any(k in b_keys for k in keys) if b_keys else not is_a
        both += is_a and is_b
        out += not is_a and not is_b
        side.append(0 if is_a == is_b else 1 if is_a else 2)
    na, nb = side.count(1), side.count(2)
    if not na or not nb:
        raise ValueError("side %s is empty" % ('A' if not na else 'B'))
    return side, (na, nb, both, out)


# ---- the command -------------------------------------------------------------------------

def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def contrast_csv(text, meta_text, by='year', a_keys=(), b_keys=(), unit='region', min_words=6,
                 max_gap=0, min_works=1, min_quoting=5, permutations=1000, seed=0):
    """The bytes `ao3.py contrast` writes for a match CSV's and a metadata CSV's text:
    (contrast, contrast-sides, contrast-permutations)."""
    if min_works < 1 or max_gap < 0 or not a_keys:
        raise ValueError("min_works at least 1, max_gap at least 0, at least one --a")
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
        return _csv([UNIT_FIELDS]), _csv([SIDE_FIELDS]), _csv([PERMUTATION_FIELDS])
    side, (na, nb, both, out) = sides_of(names, meta, by, a_keys, b_keys)
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
    units, perms, _ = contrast(recs, len(names), n_script, unit_of, len(about), side, min_words,
                               max_gap, min_quoting, permutations, seed, 32)
    n, P = na + nb, permutations
    family = [u for u, v in enumerate(units) if v['adj_ge'] != NONE]
    family.sort(key=lambda u: (units[u]['adj_ge'], -units[u]['statistic'], u))
    utab = [UNIT_FIELDS]
    for u in family:
        v = units[u]
        a, b = v['a_works'], v['b_works']
        appm, bppm = a * 1000000 // na, b * 1000000 // nb
        lo, hi = min(appm, bppm), max(appm, bppm)
        utab.append([u + 1] + list(about[u][:4])
                    + [a, b, appm, bppm, (a + b) * na * 1000 // n,
                       'A' if v['d'] > 0 else 'B' if v['d'] < 0 else '=',
                       hi * 1000 // lo if lo else '', v['statistic'], v['ge'],
                       (v['ge'] + 1) * 1000000 // (P + 1), v['adj_ge'],
                       (v['adj_ge'] + 1) * 1000000 // (P + 1), about[u][4]])
    active = [bool(c) for c in cov]
    stab = [SIDE_FIELDS]
    for name, code, keys, works in (('A', 1, '; '.join(a_keys), na),
                                    ('B', 2, '; '.join(b_keys) if b_keys else EVERY_OTHER, nb)):
        mine = sum(1 for w, s in enumerate(side) if s == code and active[w])
        quoted = sum(1 for u in family if units[u]['a_works' if code == 1 else 'b_works'])
        stab.append([name, keys, works, mine, quoted])
    is_a = [any(k in a_keys for k in (gr.keys_of(meta[gr.stem(nm)], by) if gr.stem(nm) in meta
                                       else ['(no metadata)'])) for nm in names]
    for name, works, want in (('BOTH', both, True), ('OUT', out, False)):
        mine = sum(1 for w, s in enumerate(side) if s == 0 and is_a[w] == want and active[w])
        stab.append([name, '', works, mine, ''])
    ptab = [PERMUTATION_FIELDS]
    for r, p in enumerate(perms):
        ptab.append([r + 1, p['a_active'], p['max_statistic'],
                     '' if p['max_unit'] == NONE else p['max_unit'] + 1])
    return _csv(utab), _csv(stab), _csv(ptab)
