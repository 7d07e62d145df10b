"""The `pairs` contract restated in plain Python, a set of script words per work: the oracle
of the tests (tests/test_pairs_host.py, tests/test_gpu_pairs.py) and of the committed
tests/golden/pairs_*.csv.  The product never imports it."""

import csv
import io

from tests import passages_restated as pr
from tests import quotes_restated as qr

NONE = 0xFFFFFFFF
PAIR_FIELDS = ['FAN_WORK_FILENAME_A', 'FAN_WORK_FILENAME_B', 'COVERED_WORDS_A',
               'COVERED_WORDS_B', 'SHARED_WORDS', 'FIRST_SHARED_WORD_INDEX',
               'LAST_SHARED_WORD_INDEX', 'LONGEST_RUN_START', 'LONGEST_RUN_WORDS',
               'LONGEST_RUN_CHARACTER', 'LONGEST_RUN_SCENE', 'LONGEST_RUN_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'PARTNERS', 'BEST_PARTNER',
               'BEST_SHARED_WORDS']
WORK_KEYS = ['covered', 'partners', 'best', 'best_shared']
PAIR_KEYS = ['a', 'b', 'shared', 'first', 'last', 'run_first', 'run_words']
UNKNOWN_WORD = '[?]'


def coverage(records, n_works, min_words=6, max_gap=0):
    """The set of script words the passages of each work cover."""
    cov = [set() for _ in range(n_works)]
    records = [tuple(r[:3]) + (0.0, 0.0) for r in records]   # (distances play no part)
    for w, a, b in qr.spans(records, min_words, max_gap):    # (raises on unsorted records)
        cov[w].update(range(a, b + 1))
    return cov


def longest_run(words):
    """(start, length) of the longest stretch of consecutive integers in the set `words`, the
    first one among equals."""
    best = (0, 0)
    start = prev = None
    for o in sorted(words):
        if prev is None or o != prev + 1:
            start = o
        prev = o
        if o - start + 1 > best[1]:
            best = (start, o - start + 1)
    return best


def pairs(records, n_works, n_script, min_words=6, max_gap=0, min_shared=6):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).
    Returns (one dict of WORK_KEYS per work, one dict of PAIR_KEYS per kept pair in (a, b)
    order)."""
    if min_words < 1 or min_shared < 1:
        raise ValueError("min_words and min_shared must be at least 1")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = coverage(records, n_works, min_words, max_gap)
    works = [dict(covered=len(c), partners=0, best=NONE, best_shared=0) for c in cov]
    active = [w for w in range(n_works) if cov[w]]
    out = []
    for i, a in enumerate(active):
        for b in active[i + 1:]:
            both = cov[a] & cov[b]
            if len(both) < min_shared:
                continue
            run = longest_run(both)
            out.append(dict(a=a, b=b, shared=len(both), first=min(both), last=max(both),
                            run_first=run[0], run_words=run[1]))
            for w, other in ((a, b), (b, a)):
                works[w]['partners'] += 1
                # the largest shared, the smaller work number on a tie
                if (len(both), -other) > (works[w]['best_shared'], -works[w]['best']):
                    works[w]['best'], works[w]['best_shared'] = other, len(both)
    return works, out


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def pairs_csv(text, min_words=6, max_gap=0, min_shared=6):
    """The bytes `ao3.py pairs` writes for a match CSV's text: (pairs, pairs-works)."""
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
    works, found = pairs(recs, len(names), n_script, min_words, max_gap, min_shared)
    unknown = (UNKNOWN_WORD, '', '')
    ptab = [PAIR_FIELDS]
    for p in sorted(found, key=lambda p: (-p['shared'], p['a'], p['b'])):
        s, n = p['run_first'], p['run_words']
        ptab.append([names[p['a']], names[p['b']], works[p['a']]['covered'],
                     works[p['b']]['covered'], p['shared'], p['first'], p['last'], s, n,
                     label.get(s, unknown)[1], label.get(s, unknown)[2],
                     ' '.join(label.get(o, unknown)[0] for o in range(s, s + n))])
    wtab = [WORK_FIELDS]
    for w, v in enumerate(works):
        if v['covered']:
            wtab.append([names[w], v['covered'], v['partners'],
                         '' if v['best'] == NONE else names[v['best']], v['best_shared']])
    return _csv(ptab), _csv(wtab)
