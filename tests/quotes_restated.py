"""The `quotes` contract restated in plain Python, word by word: the oracle of the tests
(tests/test_quotes_host.py, tests/test_gpu_quotes.py) and of the committed
tests/golden/quotes_*.csv.  The product never imports it."""

import csv
import io

from tests import passages_restated as pr

NONE = 0xFFFFFFFF
REGION_FIELDS = ['ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'WORDS',
                 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'PASSAGES', 'WORKS',
                 'MATCHED_WORDS', 'EXACT_WORDS', 'PEAK_WORKS', 'PEAK_WORD_START',
                 'PEAK_WORD_END', 'ORIGINAL_SCRIPT_TEXT']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'MATCHED_WORDS',
               'EXACT_WORDS', 'WORKS', 'PASSAGES', 'PASSAGE_WORKS', 'REGION']
WORD_KEYS = ['n_words', 'n_exact', 'n_works', 'n_passages', 'n_passage_works', 'region']
REGION_KEYS = ['first', 'last', 'n_passages', 'n_works', 'n_words', 'n_exact', 'peak',
               'peak_first', 'peak_last']
UNKNOWN_WORD = '[?]'


def spans(records, min_words=6, max_gap=0):
    """(work, first script word, last script word) of every passage."""
    out = []
    for p in pr.passages(records, min_words, max_gap):       # (raises on unsorted records)
        a, b = records[p['first']], records[p['first'] + p['n_words'] - 1]
        assert a[0] == b[0] and a[2] <= b[2]
        out.append((a[0], a[2], b[2]))
    return out


def quotes(records, n_works, n_script, min_words=6, max_gap=0, min_works=1):
    """records: (work, fan_ix, orig_ix, dist, comb) tuples sorted by (work, fan_ix).
    Returns (one dict of WORD_KEYS per script word, one dict of REGION_KEYS per region)."""
    if min_words < 1 or min_works < 1:
        raise ValueError("min_words and min_works must be at least 1")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    n_words, n_exact = [0] * n_script, [0] * n_script
    works_at = [set() for _ in range(n_script)]
    for w, _, o, _, comb in records:
        n_words[o] += 1
        n_exact[o] += 1 if comb <= 0 else 0
        works_at[o].add(w)
    found = spans(records, min_words, max_gap)
    n_passages = [0] * n_script
    covering = [set() for _ in range(n_script)]
    for w, a, b in found:
        for o in range(a, b + 1):
            n_passages[o] += 1
            covering[o].add(w)
    depth = [len(s) for s in covering]
    region = [NONE] * n_script
    bounds = []
    for o in range(n_script):
        if depth[o] < min_works:
            continue
        if o and region[o - 1] != NONE:
            bounds[-1][1] = o
        else:
            bounds.append([o, o])
        region[o] = len(bounds) - 1
    r_passages = [0] * len(bounds)
    r_works = [set() for _ in bounds]
    for w, a, b in found:
        for k in sorted(set(region[o] for o in range(a, b + 1)) - {NONE}):
            r_passages[k] += 1
            r_works[k].add(w)
    words = [dict(n_words=n_words[o], n_exact=n_exact[o], n_works=len(works_at[o]),
                  n_passages=n_passages[o], n_passage_works=depth[o], region=region[o])
             for o in range(n_script)]
    regions = []
    for k, (a, b) in enumerate(bounds):
        peak = max(depth[a:b + 1])
        pf = next(o for o in range(a, b + 1) if depth[o] == peak)
        pl = pf
        while pl < b and depth[pl + 1] == peak:
            pl += 1
        regions.append(dict(first=a, last=b, n_passages=r_passages[k], n_works=len(r_works[k]),
                            n_words=sum(n_words[a:b + 1]), n_exact=sum(n_exact[a:b + 1]),
                            peak=peak, peak_first=pf, peak_last=pl))
    return words, regions


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def quotes_csv(text, min_words=6, max_gap=0, min_works=1):
    """The bytes `ao3.py quotes` writes for a match CSV's text: (quotes, quotes-words)."""
    rows = pr.read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4]), pr._num(rows[k][9]), pr._num(rows[k][11]))
            for w, f, k in keyed]
    label = {}
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        if label.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
    n_script = max(label) + 1 if label else 0
    words, regions = quotes(recs, len(work_of), n_script, min_words, max_gap, min_works)

    def text_of(o):
        return label[o][0] if o in label else UNKNOWN_WORD
    rtab = [REGION_FIELDS]
    for r in regions:
        a, b = r['first'], r['last']
        rtab.append([a, b, b - a + 1, label[a][1], label[a][2], r['n_passages'], r['n_works'],
                     r['n_words'], r['n_exact'], r['peak'], r['peak_first'], r['peak_last'],
                     ' '.join(text_of(o) for o in range(a, b + 1))])
    wtab = [WORD_FIELDS]
    for o, w in enumerate(words):
        if w['n_words'] or w['n_passages']:
            wtab.append([o, text_of(o), w['n_words'], w['n_exact'], w['n_works'],
                         w['n_passages'], w['n_passage_works'],
                         '' if w['region'] == NONE else w['region'] + 1])
    return _csv(rtab), _csv(wtab)
