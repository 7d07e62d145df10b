"""The `sources` contract restated in plain Python, passage against passage: the oracle of the
tests (tests/test_sources_host.py, tests/test_gpu_sources.py) and of the committed
tests/golden/sources_trilogy.*.csv.  Quadratic and obvious.  The product never imports it."""

import csv
import io

from tests.passages_restated import passages as restated_passages, read_rows

PASSAGE_FIELDS = ['SCRIPT', 'FAN_WORK_FILENAME', 'FAN_WORK_WORD_START', 'FAN_WORK_WORD_END',
                  'ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'MATCHED_WORDS',
                  'EXACT_WORDS', 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'RIVALS',
                  'RIVAL_SCRIPTS', 'CONTESTED_WORDS', 'SOLE_WORDS', 'OUTCOME', 'BEST_RIVAL',
                  'BEST_RIVAL_WORDS', 'BEST_RIVAL_FAN_START', 'FAN_WORK_TEXT',
                  'ORIGINAL_SCRIPT_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'SCRIPT', 'PASSAGES', 'ALONE', 'WON', 'LOST', 'COVERED_WORDS',
               'CONTESTED_WORDS', 'SOLE_WORDS', 'WORK_SCRIPTS', 'PRIMARY']
SCRIPT_FIELDS = ['SCRIPT', 'WORKS', 'PASSAGES', 'ALONE', 'WON', 'LOST', 'COVERED_WORDS',
                 'CONTESTED_WORDS', 'SOLE_WORDS', 'PRIMARY_WORKS']
PAIR_FIELDS = ['SCRIPT_A', 'SCRIPT_B', 'WORKS_BOTH', 'CONTESTS', 'SHARED_WORDS', 'A_WINS',
               'B_WINS']
ALONE, WON, LOST = 'alone', 'won', 'lost'


def key(p):
    return (p['n_words'], p['n_exact'], -p['script'])


def overlap(p, q):
    return min(p['fan_last'], q['fan_last']) - max(p['fan_first'], q['fan_first']) + 1


def is_rival(p, q):
    return (q['script'] != p['script'] and q['work'] == p['work']
            and q['fan_first'] <= p['fan_last'] and p['fan_first'] <= q['fan_last'])


def sources(files, min_words=6, max_gap=0):
    """files[s]: the records of script s as (work, fan_ix, orig_ix, dist, comb) tuples sorted by
    (work, fan_ix), the work numbers shared by all files.  Returns dict(passages, works,
    scripts, pairs), lists of dicts with the fields of fs_source_passage, fs_source_work,
    fs_source_script and fs_source_pair, in their orders."""
    K = len(files)
    every = []
    for s, recs in enumerate(files):
        for p in restated_passages(recs, min_words, max_gap):
            a, n = p['first'], p['n_words']
            every.append(dict(script=s, work=recs[a][0], first=a, n_words=n,
                              n_exact=p['n_exact'], fan_first=recs[a][1],
                              fan_last=recs[a + n - 1][1], orig_first=recs[a][2],
                              orig_last=recs[a + n - 1][2]))
    every.sort(key=lambda p: (p['work'], p['fan_first'], p['script'], p['first']))
    in_work = {}
    for p in every:
        in_work.setdefault(p['work'], []).append(p)
    for p in every:
        rivals = [q for q in in_work[p['work']] if is_rival(p, q)]
        words = set()
        for q in rivals:
            lo, hi = max(p['fan_first'], q['fan_first']), min(p['fan_last'], q['fan_last'])
            if hi - lo > 1 << 20:
                raise ValueError("the oracle lists the words of a span")
            words.update(range(lo, hi + 1))
        span = p['fan_last'] - p['fan_first'] + 1
        p['rivals'] = len(rivals)
        p['rival_scripts'] = len({q['script'] for q in rivals})
        p['contested_words'] = len(words)
        p['sole_words'] = span - len(words)
        p['outcome'] = (ALONE if not rivals
                        else WON if all(key(p) > key(q) for q in rivals) else LOST)
        p['best_rival'] = p['best_rival_words'] = p['best_rival_fan_first'] = None
        if rivals:
            best = max(rivals, key=lambda q: key(q) + (-q['fan_first'], -q['first']))
            p['best_rival'] = best['script']
            p['best_rival_words'] = best['n_words']
            p['best_rival_fan_first'] = best['fan_first']
    works = []
    for w in sorted({p['work'] for p in every}):
        here = [p for p in every if p['work'] == w]
        rows = []
        for s in sorted({p['script'] for p in here}):
            mine = [p for p in here if p['script'] == s]
            rows.append(dict(work=w, script=s, passages=len(mine),
                             alone=sum(p['outcome'] == ALONE for p in mine),
                             won=sum(p['outcome'] == WON for p in mine),
                             lost=sum(p['outcome'] == LOST for p in mine),
                             covered_words=sum(p['fan_last'] - p['fan_first'] + 1 for p in mine),
                             contested_words=sum(p['contested_words'] for p in mine),
                             sole_words=sum(p['sole_words'] for p in mine)))
        most = max(r['covered_words'] for r in rows)
        first = min(r['script'] for r in rows if r['covered_words'] == most)
        for r in rows:
            r['work_scripts'] = len(rows)
            r['primary'] = int(r['script'] == first)
        works.extend(rows)
    scripts = []
    for s in range(K):
        rows = [r for r in works if r['script'] == s]
        d = dict(works=len(rows), primary_works=sum(r['primary'] for r in rows))
        for k in ('passages', 'alone', 'won', 'lost', 'covered_words', 'contested_words',
                  'sole_words'):
            d[k] = sum(r[k] for r in rows)
        scripts.append(d)
    pairs = []
    for a in range(K):
        for b in range(a + 1, K):
            met = [(p, q) for p in every if p['script'] == a
                   for q in in_work[p['work']] if q['script'] == b and is_rival(p, q)]
            wins = sum(key(p) > key(q) for p, q in met)
            pairs.append(dict(a=a, b=b,
                              works_both=len({r['work'] for r in works if r['script'] == a}
                                             & {r['work'] for r in works if r['script'] == b}),
                              contests=len(met), shared_words=sum(overlap(p, q) for p, q in met),
                              a_wins=wins, b_wins=len(met) - wins))
    return dict(passages=every, works=works, scripts=scripts, pairs=pairs)


PASSAGE_KEYS = ['script', 'work', 'first', 'n_words', 'n_exact', 'fan_first', 'fan_last',
                'orig_first', 'orig_last', 'rivals', 'rival_scripts', 'outcome', 'best_rival',
                'best_rival_words', 'best_rival_fan_first', 'reserved', 'contested_words',
                'sole_words']
WORK_KEYS = ['work', 'script', 'passages', 'alone', 'won', 'lost', 'work_scripts', 'primary',
             'covered_words', 'contested_words', 'sole_words']
SCRIPT_KEYS = ['works', 'passages', 'alone', 'won', 'lost', 'primary_works', 'covered_words',
               'contested_words', 'sole_words']
PAIR_KEYS = ['a', 'b', 'works_both', 'reserved', 'contests', 'shared_words', 'a_wins', 'b_wins']


def as_tuples(got):
    """The four lists of sources() as tuples in the field order of the four structs: outcome
    0, 1, 2 for alone, won, lost; no best rival as 0xFFFFFFFF, 0, 0; reserved 0."""
    def passage(p):
        d = dict(p, reserved=0, outcome=(ALONE, WON, LOST).index(p['outcome']))
        if p['best_rival'] is None:
            d.update(best_rival=0xFFFFFFFF, best_rival_words=0, best_rival_fan_first=0)
        return tuple(d[k] for k in PASSAGE_KEYS)
    return ([passage(p) for p in got['passages']],
            [tuple(r[k] for k in WORK_KEYS) for r in got['works']],
            [tuple(r[k] for k in SCRIPT_KEYS) for r in got['scripts']],
            [tuple(dict(r, reserved=0)[k] for k in PAIR_KEYS) for r in got['pairs']])


def _num(text):
    return float(text) if text != '' else float('nan')


def number_works(rows_of):
    """{FAN_WORK_FILENAME: number}: first appearance through the files in turn."""
    number = {}
    for rows in rows_of:
        for r in rows:
            number.setdefault(r[0], len(number))
    return number


def sorted_file(rows, number):
    """(text rows, records) of one file in stable (global work, FAN_WORK_WORD_INDEX) order."""
    keyed = sorted(((number[r[0]], int(r[1]), k) for k, r in enumerate(rows)),
                   key=lambda t: (t[0], t[1]))          # stable: ties keep file order
    srt = [rows[k] for _, _, k in keyed]
    recs = [(w, f, int(rows[k][4]), _num(rows[k][9]), _num(rows[k][11])) for w, f, k in keyed]
    return srt, recs


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def sources_csv(texts, names, min_words=6, max_gap=0):
    """The text of the four files `ao3.py sources` writes for the match CSVs' texts and the
    scripts' names: (passages, works, scripts, pairs)."""
    rows_of = [read_rows(t) for t in texts]
    number = number_works(rows_of)
    work_names = list(number)
    both = [sorted_file(rows, number) for rows in rows_of]
    got = sources([recs for _, recs in both], min_words, max_gap)
    ptab = [PASSAGE_FIELDS]
    for p in got['passages']:
        part = both[p['script']][0][p['first']:p['first'] + p['n_words']]
        alone = p['outcome'] == ALONE
        ptab.append([names[p['script']], work_names[p['work']], p['fan_first'], p['fan_last'],
                     p['orig_first'], p['orig_last'], p['n_words'], p['n_exact'], part[0][7],
                     part[0][8], p['rivals'], p['rival_scripts'], p['contested_words'],
                     p['sole_words'], p['outcome'],
                     '' if alone else names[p['best_rival']],
                     '' if alone else p['best_rival_words'],
                     '' if alone else p['best_rival_fan_first'],
                     ' '.join(r[2] for r in part), ' '.join(r[5] for r in part)])
    wtab = [WORK_FIELDS] + [
        [work_names[r['work']], names[r['script']], r['passages'], r['alone'], r['won'],
         r['lost'], r['covered_words'], r['contested_words'], r['sole_words'],
         r['work_scripts'], r['primary']] for r in got['works']]
    stab = [SCRIPT_FIELDS] + [
        [names[s], r['works'], r['passages'], r['alone'], r['won'], r['lost'],
         r['covered_words'], r['contested_words'], r['sole_words'], r['primary_works']]
        for s, r in enumerate(got['scripts'])]
    qtab = [PAIR_FIELDS] + [
        [names[r['a']], names[r['b']], r['works_both'], r['contests'], r['shared_words'],
         r['a_wins'], r['b_wins']] for r in got['pairs']]
    return _csv(ptab), _csv(wtab), _csv(stab), _csv(qtab)
