"""The `digest` contract restated in plain Python from its definitions: the oracle of the tests
(tests/test_digest_host.py, tests/test_gpu_digest.py) and of the committed
tests/golden/digest_*.csv.  The product never imports it.

A set of script words per work (tests/pairs_restated.py), the greedy loop as the definition
words it, with max over (gain, -work), and every per-work figure by brute force over the sets:
no bounds, no tiles, no bit rows."""

import csv
import io

from tests import pairs_restated as plr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
PICK_FIELDS = ['RANK', 'FAN_WORK_FILENAME', 'COVERED_WORDS', 'NEW_WORDS', 'NEW_RUNS',
               'LONGEST_NEW_FIRST_WORD_INDEX', 'LONGEST_NEW_LAST_WORD_INDEX', 'LONGEST_NEW_WORDS',
               'CHARACTER', 'SCENE', 'CUM_WORDS', 'CUM_PERCENT', 'SUBSUMED_WORKS',
               'CUM_SUBSUMED_WORKS', 'REPRESENTED_WORKS', 'LONGEST_NEW_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'PICK_RANK', 'IN_PICKS_WORDS',
               'IN_PICKS_PERCENT', 'SUBSUMED_AT', 'BEST_PICK', 'BEST_PICK_FILENAME',
               'BEST_PICK_SHARED']
PICK_KEYS = ['work', 'covered', 'new_words', 'new_runs', 'longest_first', 'longest_words',
             'cum_words']
WORK_KEYS = ['work', 'covered', 'pick_rank', 'in_picks', 'subsumed_at', 'best_pick',
             'best_shared']
UNKNOWN_WORD = '[?]'


def runs_of(words):
    """The maximal stretches (first, length) of consecutive integers in the set `words`."""
    out = []
    for o in sorted(words):
        if out and out[-1][0] + out[-1][1] == o:
            out[-1][1] += 1
        else:
            out.append([o, 1])
    return [tuple(r) for r in out]


def digest(records, n_works, n_script, min_words=6, max_gap=0, picks=0, cover=100, min_gain=1):
    """records: (work, fan_ix, orig_ix) tuples sorted by (work, fan_ix).  Returns (one dict of
    PICK_KEYS per pick in pick order, one dict of WORK_KEYS per active work in work order,
    TOTAL)."""
    if min_words < 1 or min_gain < 1 or not 1 <= cover <= 100 or picks < 0:
        raise ValueError("min_words and min_gain at least 1, cover from 1 to 100, picks from 0")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = plr.coverage(records, n_works, min_words, max_gap)
    active = [w for w in range(n_works) if cov[w]]
    union = set()
    for w in active:
        union |= cov[w]
    total = len(union)
    have, stamp, found = set(), {}, []
    while active:
        r = len(found) + 1
        if picks and r - 1 == picks:
            break
        gain, minus = max((len(cov[w] - have), -w) for w in active)
        if gain < min_gain:
            break
        if len(have) * 100 >= cover * total:
            break
        w = -minus
        new = cov[w] - have
        have |= new
        for o in new:
            stamp[o] = r
        runs = runs_of(new)
        first, words = max(runs, key=lambda run: (run[1], -run[0]))
        found.append(dict(work=w, covered=len(cov[w]), new_words=len(new), new_runs=len(runs),
                          longest_first=first, longest_words=words, cum_words=len(have)))
    rank_of = {p['work']: k + 1 for k, p in enumerate(found)}
    works = []
    for w in active:
        inside = cov[w] & have
        best, shared = NONE, 0
        for k, p in enumerate(found):
            both = len(cov[w] & cov[p['work']])
            if both > shared:                           # (the earlier pick on a tie)
                best, shared = k + 1, both
        works.append(dict(work=w, covered=len(cov[w]), pick_rank=rank_of.get(w, NONE),
                          in_picks=len(inside),
                          subsumed_at=max(stamp[o] for o in cov[w]) if inside == cov[w] else NONE,
                          best_pick=best, best_shared=shared))
    return found, works, total


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def digest_csv(text, min_words=6, max_gap=0, picks=0, cover=100, min_gain=1):
    """The bytes `ao3.py digest` writes for a match CSV's text: (digest, digest-works)."""
    rows = pr.read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4])) for w, f, k in keyed]
    names = list(work_of)
    label = {}
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        if label.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
    n_script = max(label) + 1 if label else 0
    found, works, total = digest(recs, len(names), n_script, min_words, max_gap, picks, cover,
                                 min_gain)
    unknown = (UNKNOWN_WORD, '', '')
    ptab = [PICK_FIELDS]
    so_far = 0
    for k, p in enumerate(found):
        a, n = p['longest_first'], p['longest_words']
        subsumed = sum(1 for v in works if v['subsumed_at'] == k + 1)
        so_far += subsumed
        ptab.append([k + 1, names[p['work']], p['covered'], p['new_words'], p['new_runs'], a,
                     a + n - 1, n, label.get(a, unknown)[1], label.get(a, unknown)[2],
                     p['cum_words'], p['cum_words'] * 100 // total, subsumed, so_far,
                     sum(1 for v in works if v['best_pick'] == k + 1),
                     ' '.join(label.get(o, unknown)[0] for o in range(a, a + n))])
    wtab = [WORK_FIELDS]
    for v in works:
        none = v['best_pick'] == NONE
        wtab.append([names[v['work']], v['covered'],
                     '' if v['pick_rank'] == NONE else v['pick_rank'], v['in_picks'],
                     v['in_picks'] * 100 // v['covered'],
                     '' if v['subsumed_at'] == NONE else v['subsumed_at'],
                     '' if none else v['best_pick'],
                     '' if none else names[found[v['best_pick'] - 1]['work']],
                     v['best_shared']])
    return _csv(ptab), _csv(wtab)
