"""The `passages` contract restated in plain Python, record by record: the oracle of the
tests (tests/test_passages_host.py, tests/test_gpu_passages.py) and of the committed
tests/golden/passages_*.csv.  The product never imports it."""

import csv
import io
import math

MATCH_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'FAN_WORK_WORD', 'FAN_WORK_ORTH_ID',
                'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_ORTH_ID',
                'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'BEST_MATCH_DISTANCE',
                'BEST_LEVENSHTEIN_DISTANCE', 'BEST_COMBINED_DISTANCE']

PASSAGE_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_START', 'FAN_WORK_WORD_END',
                  'ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'MATCHED_WORDS',
                  'EXACT_WORDS', 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE',
                  'MEAN_MATCH_DISTANCE', 'MAX_MATCH_DISTANCE', 'MEAN_COMBINED_DISTANCE',
                  'MAX_COMBINED_DISTANCE', 'FAN_WORK_TEXT', 'ORIGINAL_SCRIPT_TEXT']


def _max(values):
    best = float('nan')
    for v in values:
        if math.isnan(v):
            continue
        if math.isnan(best) or v > best:
            best = v
    return best


def passages(records, min_words=6, max_gap=0):
    """records: (work, fan_ix, orig_ix, dist, comb) tuples sorted by (work, fan_ix).
    Returns dicts with the fields of fs_passage."""
    runs = []
    for i, s in enumerate(records):
        if runs:
            r = records[i - 1]
            if (s[0], s[1]) < (r[0], r[1]):
                raise ValueError("records out of (work, fan_ix) order at %d" % i)
            df = s[1] - r[1]
            do = s[2] - r[2]
            if s[0] == r[0] and 1 <= df <= 1 + max_gap and 1 <= do <= 1 + max_gap:
                runs[-1].append(i)
                continue
        runs.append([i])
    out = []
    for run in runs:
        if len(run) < min_words:
            continue
        dists = [records[i][3] for i in run]
        combs = [records[i][4] for i in run]
        dist_sum = 0.0
        for v in dists:
            dist_sum += v
        comb_sum = 0.0
        for v in combs:
            comb_sum += v
        out.append(dict(first=run[0], n_words=len(run),
                        n_exact=sum(1 for c in combs if c <= 0),
                        dist_sum=dist_sum, dist_max=_max(dists),
                        comb_sum=comb_sum, comb_max=_max(combs)))
    return out


def read_rows(text):
    """Text rows of a match CSV (dated file with header, or batch file without)."""
    rows = [r for r in csv.reader(io.StringIO(text, newline=''))]
    if rows and rows[0] == MATCH_FIELDS:
        rows = rows[1:]
    return rows


def _num(text):
    return float(text) if text != '' else float('nan')


def passages_csv(text, min_words=6, max_gap=0):
    """The bytes `ao3.py passages` writes for a match CSV's text."""
    rows = read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    srt = [rows[k] for _, _, k in keyed]
    recs = [(w, f, int(rows[k][4]), _num(rows[k][9]), _num(rows[k][11])) for w, f, k in keyed]
    out = [PASSAGE_FIELDS]
    for p in passages(recs, min_words, max_gap):
        a, n = p['first'], p['n_words']
        part = srt[a:a + n]
        out.append([part[0][0], recs[a][1], recs[a + n - 1][1], recs[a][2], recs[a + n - 1][2],
                    n, p['n_exact'], part[0][7], part[0][8],
                    p['dist_sum'] / n, p['dist_max'], p['comb_sum'] / n, p['comb_max'],
                    ' '.join(r[2] for r in part), ' '.join(r[5] for r in part)])
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(out)
    return buf.getvalue()
