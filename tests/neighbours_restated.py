"""The `neighbours` contract restated in plain Python, a set of script words per work and a dict
of weights: the oracle of the tests (tests/test_neighbours_host.py,
tests/test_gpu_neighbours.py) and of the committed tests/golden/neighbours_*.csv.  The product
never imports it, and it imports nothing of the product."""

import csv
import io

from tests import passages_restated as pr
from tests import quotes_restated as qr

NONE = 0xFFFFFFFF
MAX_TOP = 32
NEIGHBOUR_FIELDS = ['FAN_WORK_FILENAME', 'RANK', 'NEIGHBOUR_FILENAME', 'SIMILARITY_PPM', 'SCORE',
                    'OWN_SCORE', 'NEIGHBOUR_OWN_SCORE', 'SHARED_WORDS', 'COVERED_WORDS',
                    'NEIGHBOUR_COVERED_WORDS', 'MUTUAL', 'BACK_RANK', 'RAREST_WORD_INDEX',
                    'RAREST_WORD', 'RAREST_DEPTH', 'RAREST_WEIGHT', 'RUN_FIRST_WORD_INDEX',
                    'RUN_WORDS', 'CHARACTER', 'SCENE', 'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'OWN_SCORE', 'RARITY_MILLI', 'CANDIDATES',
               'LISTED', 'LISTED_BY', 'MUTUAL', 'NEAREST', 'NEAREST_PPM']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'CHARACTER', 'SCENE',
               'DEPTH', 'WEIGHT']
NEIGHBOUR_KEYS = ['a', 'b', 'rank', 'back_rank', 'ppm', 'score', 'shared', 'rarest',
                  'rarest_depth', 'rarest_weight', 'run_first', 'run_words']
WORK_KEYS = ['covered', 'own', 'candidates', 'listed', 'listed_by', 'mutual', 'nearest',
             'nearest_ppm']
WORD_KEYS = ['depth', 'weight']
UNKNOWN_WORD = '[?]'


def weight_of(n_active, depth, weight='rarity'):
    """The weight of a script word `depth` of the `n_active` active works cover."""
    if weight not in ('rarity', 'flat'):
        raise ValueError("weight is rarity or flat")
    if depth == 0:
        return 0
    return 1 if weight == 'flat' else (n_active // depth).bit_length()


def coverage(records, n_works, min_words=6, max_gap=0):
    """The set of script words the passages of each work cover."""
    cov = [set() for _ in range(n_works)]
    records = [tuple(r[:3]) + (0.0, 0.0) for r in records]   # (distances play no part)
    for w, a, b in qr.spans(records, min_words, max_gap):    # (raises on unsorted records)
        cov[w].update(range(a, b + 1))
    return cov


def run_around(words, o):
    """(start, length) of the maximal stretch of consecutive integers of the set `words` that
    holds `o`."""
    a = b = o
    while a - 1 in words:
        a -= 1
    while b + 1 in words:
        b += 1
    return a, b - a + 1


def neighbours(records, n_works, n_script, min_words=6, max_gap=0, weight='rarity', top=10,
               min_score=1, min_similarity=0):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).  Returns (one dict
    of WORK_KEYS per work, one dict of WORD_KEYS per script word, one dict of NEIGHBOUR_KEYS per
    listed pair in (work, rank) order)."""
    if min_words < 1 or min_score < 1:
        raise ValueError("min_words and min_score must be at least 1")
    if not 1 <= top <= MAX_TOP:
        raise ValueError("top is from 1 to 32")
    if not 0 <= min_similarity <= 100:
        raise ValueError("min_similarity is a whole percentage")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = coverage(records, n_works, min_words, max_gap)
    active = [w for w in range(n_works) if cov[w]]
    depth = [0] * n_script
    for w in active:
        for o in cov[w]:
            depth[o] += 1
    wt = [weight_of(len(active), d, weight) for d in depth]
    words = [dict(depth=d, weight=x) for d, x in zip(depth, wt)]
    own = [sum(wt[o] for o in c) for c in cov]
    works = [dict(covered=len(c), own=s, candidates=0, listed=0, listed_by=0, mutual=0,
                  nearest=NONE, nearest_ppm=0) for c, s in zip(cov, own)]
    lists = {}
    for a in active:
        found = []
        for b in active:
            if b == a:
                continue
            score = sum(wt[o] for o in cov[a] & cov[b])
            if score < min_score:
                continue
            ppm = score * 1000000 // (own[a] + own[b] - score)
            if ppm < min_similarity * 10000:
                continue
            found.append(((ppm << 32) | (0xFFFFFFFF - b), b, ppm, score))
        found.sort(reverse=True)
        works[a]['candidates'] = len(found)
        lists[a] = found[:top]
    out = []
    for a in active:
        for rank, (_, b, ppm, score) in enumerate(lists[a], 1):
            both = cov[a] & cov[b]
            rare = min(both, key=lambda o: (-wt[o], o))      # the first among equals
            run = run_around(both, rare)
            back = [k for k, e in enumerate(lists[b], 1) if e[1] == a]
            out.append(dict(a=a, b=b, rank=rank, back_rank=back[0] if back else NONE, ppm=ppm,
                            score=score, shared=len(both), rarest=rare,
                            rarest_depth=depth[rare], rarest_weight=wt[rare], run_first=run[0],
                            run_words=run[1]))
            works[a]['listed'] += 1
            works[b]['listed_by'] += 1
            works[a]['mutual'] += bool(back)
            if rank == 1:
                works[a]['nearest'], works[a]['nearest_ppm'] = b, ppm
    return works, words, out


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def read(text):
    """(records sorted by (work, fan_ix), the works' names in first-appearance order, the label
    (word, character, scene) of every script word a record names) of a match CSV's text."""
    rows = pr.read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4])) for w, f, k in keyed]
    label = {}
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        if label.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
    return recs, list(work_of), label


def neighbours_csv(text, weight='rarity', top=10, min_score=1, min_similarity=0, min_words=6,
                   max_gap=0):
    """The bytes `ao3.py neighbours` writes for a match CSV's text: (neighbours,
    neighbours-works, neighbours-words)."""
    recs, names, label = read(text)
    n_script = max(label) + 1 if label else 0
    works, words, found = neighbours(recs, len(names), n_script, min_words, max_gap, weight, top,
                                     min_score, min_similarity)
    unknown = (UNKNOWN_WORD, '', '')
    ntab = [NEIGHBOUR_FIELDS]
    for p in found:
        a, b, s, n = p['a'], p['b'], p['run_first'], p['run_words']
        mutual = p['back_rank'] != NONE
        ntab.append([names[a], p['rank'], names[b], p['ppm'], p['score'], works[a]['own'],
                     works[b]['own'], p['shared'], works[a]['covered'], works[b]['covered'],
                     int(mutual), p['back_rank'] if mutual else '', p['rarest'],
                     label.get(p['rarest'], unknown)[0], p['rarest_depth'], p['rarest_weight'],
                     s, n, label.get(s, unknown)[1], label.get(s, unknown)[2],
                     ' '.join(label.get(o, unknown)[0] for o in range(s, s + n))])
    wtab = [WORK_FIELDS]
    for w, v in enumerate(works):
        if v['covered']:
            wtab.append([names[w], v['covered'], v['own'], v['own'] * 1000 // v['covered'],
                         v['candidates'], v['listed'], v['listed_by'], v['mutual'],
                         '' if v['nearest'] == NONE else names[v['nearest']], v['nearest_ppm']])
    otab = [WORD_FIELDS]
    for o, v in enumerate(words):
        if v['depth']:
            otab.append([o] + list(label.get(o, unknown)) + [v['depth'], v['weight']])
    return _csv(ntab), _csv(wtab), _csv(otab)
