"""The `fragments` contract restated in plain Python from its definitions: the oracle of the
tests (tests/test_fragments_host.py, tests/test_gpu_fragments.py) and of the committed
tests/golden/fragments_*.csv.  The product never imports it.

S(a, b) is counted work by work from the coverage sets of tests/pairs_restated.py, and a
stretch is closed when S drops on both sides, as the definition says; the START/END tables of
the library appear nowhere here, so that their identity is what the comparison checks."""

import bisect
import csv
import io

from tests import pairs_restated as plr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
FRAGMENT_FIELDS = ['RANK', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'WORDS', 'CHARACTER', 'SCENE',
                   'WORKS', 'EXACT_WORKS', 'LEFT_DROP', 'RIGHT_DROP', 'FIRST_FAN_WORK_FILENAME',
                   'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'RUNS', 'COVERED_WORDS', 'HELD_FRAGMENTS', 'EXACT_FRAGMENTS',
               'LONGEST_FIRST_WORD_INDEX', 'LONGEST_LAST_WORD_INDEX', 'LONGEST_WORDS',
               'LONGEST_WORKS', 'LONGEST_TEXT']
FRAGMENT_KEYS = ['first', 'last', 'works', 'exact_works', 'start_works', 'end_works',
                 'first_work']
WORK_KEYS = ['work', 'runs', 'covered', 'held', 'exact', 'longest_first', 'longest_last',
             'longest_works']
UNKNOWN_WORD = '[?]'


class Support(object):
    """S(a, b) over coverage sets: per script word a the works covering it, each with the
    number of consecutive words it covers from a on, sorted."""

    def __init__(self, cov, n_script):
        self.n_script = n_script
        self.cov = cov
        self.at = [[] for _ in range(n_script)]
        for w, words in enumerate(cov):
            reach = {}
            for o in sorted(words, reverse=True):
                reach[o] = reach.get(o + 1, 0) + 1
            for o, k in reach.items():
                self.at[o].append((k, w))
        for here in self.at:
            here.sort()

    def holders(self, a, b):
        """The works holding [a, b], in no order."""
        if a < 0 or b >= self.n_script or a > b:
            return []
        here = self.at[a]
        return [w for _, w in here[bisect.bisect_left(here, (b - a + 1, -1)):]]

    def S(self, a, b):
        return len(self.holders(a, b))

    def longest_from(self, a):
        return self.at[a][-1][0] if self.at[a] else 0


def runs_of(words):
    """The maximal stretches (first, last) of consecutive integers in the set `words`."""
    out = []
    for o in sorted(words):
        if out and out[-1][1] == o - 1:
            out[-1][1] = o
        else:
            out.append([o, o])
    return [tuple(r) for r in out]


def fragments(records, n_works, n_script, min_words=6, max_gap=0, min_works=2, min_length=3,
              max_words=128):
    """records: (work, fan_ix, orig_ix) tuples sorted by (work, fan_ix).  Returns (one dict of
    FRAGMENT_KEYS per fragment in (words, first) order, one dict of WORK_KEYS per active work in
    work order)."""
    if min_words < 1 or min_length < 1 or max_words < min_length:
        raise ValueError("min_words and min_length at least 1, max_words at least min_length")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = plr.coverage(records, n_works, min_words, max_gap)
    sup = Support(cov, n_script)
    found = []
    for a in range(n_script):
        for k in range(min_length, min(max_words, sup.longest_from(a)) + 1):
            b = a + k - 1
            held_by = sup.holders(a, b)
            s = len(held_by)
            left, right = sup.S(a - 1, b), sup.S(a, b + 1)
            if s < min_works or not (s > left and s > right):
                continue
            starting = [w for w in held_by if a - 1 not in cov[w]]
            exact = [w for w in starting if b + 1 not in cov[w]]
            found.append(dict(first=a, last=b, works=s, exact_works=len(exact),
                              start_works=s - left, end_works=s - right,
                              first_work=min(starting), holders=held_by))
    found.sort(key=lambda f: (f['last'] - f['first'], f['first']))
    listed = set((f['first'], f['last']) for f in found)
    held = [0] * n_works
    for f in found:
        for w in f.pop('holders'):
            held[w] += 1
    works = []
    for w in range(n_works):
        if not cov[w]:
            continue
        runs = runs_of(cov[w])
        lf, ll = max(runs, key=lambda r: (r[1] - r[0], -r[0]))
        k = ll - lf + 1
        works.append(dict(work=w, runs=len(runs), covered=len(cov[w]), held=held[w],
                          exact=sum(1 for r in runs if r in listed), longest_first=lf,
                          longest_last=ll,
                          longest_works=sup.S(lf, ll) if min_length <= k <= max_words else NONE))
    return found, works


def ranked(found, top=0):
    """The fragments in the order of the CSV: WORKS descending, then WORDS descending, then the
    first word; the first `top` of them (0: all)."""
    out = sorted(found, key=lambda f: (-f['works'], -(f['last'] - f['first']), f['first']))
    return out[:top] if top else out


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def fragments_csv(text, min_words=6, max_gap=0, min_works=2, min_length=3, max_words=128,
                  top=0):
    """The bytes `ao3.py fragments` writes for a match CSV's text: (fragments,
    fragments-works)."""
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
    found, works = fragments(recs, len(names), n_script, min_words, max_gap, min_works,
                             min_length, max_words)

    def text_of(a, b):
        return ' '.join(label[o][0] if o in label else UNKNOWN_WORD for o in range(a, b + 1))
    ftab = [FRAGMENT_FIELDS]
    for rank, f in enumerate(ranked(found, top)):
        a, b = f['first'], f['last']
        ftab.append([rank + 1, a, b, b - a + 1, label[a][1], label[a][2], f['works'],
                     f['exact_works'], f['start_works'], f['end_works'], names[f['first_work']],
                     text_of(a, b)])
    wtab = [WORK_FIELDS]
    for v in works:
        a, b = v['longest_first'], v['longest_last']
        wtab.append([names[v['work']], v['runs'], v['covered'], v['held'], v['exact'], a, b,
                     b - a + 1, '' if v['longest_works'] == NONE else v['longest_works'],
                     text_of(a, b)])
    return _csv(ftab), _csv(wtab)
