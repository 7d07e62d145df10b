"""Plain-Python restatement of the integer part of `ao3.py matrix`: the contract of fs_matrix in
include/fandom_search.h, written from the issue's rules over (work, fan_ix, orig_ix) tuples.
The oracle of tests/test_matrix_restated_host.py and tests/test_gpu_matrix.py; the product never
imports it."""

import collections
import csv

FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'FAN_WORK_WORD', 'FAN_WORK_ORTH_ID',
          'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_ORTH_ID',
          'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'BEST_MATCH_DISTANCE',
          'BEST_LEVENSHTEIN_DISTANCE', 'BEST_COMBINED_DISTANCE']


def sort_records(records):
    """Stable by work in first-appearance order, then by fan index; works renumbered so."""
    ids = {}
    for w, _, _ in records:
        ids.setdefault(w, len(ids))
    return sorted(((ids[w], f, o) for w, f, o in records), key=lambda r: (r[0], r[1]))


def fan_runs(records):
    """Lists of records: a run starts where the work changes or fan != previous fan + 1."""
    runs = []
    for i, r in enumerate(records):
        p = records[i - 1] if i else None
        if p is not None and (r[0], r[1]) < (p[0], p[1]):
            raise ValueError("records out of (work, fan_ix) order at %d" % i)
        if p is None or r[0] != p[0] or r[1] != p[1] + 1:
            runs.append([])
        runs[-1].append(r)
    return runs


def run_spans(run):
    """The closed intervals [a, b] of one fan run, in the order they close, from c(v) alone."""
    c = collections.Counter(o for _, _, o in run)
    out, cur = [], None
    for v in sorted(c):
        if cur is not None and cur[1] == v - 1:
            cur[1] = v
        else:
            if cur is not None:
                out.append(tuple(cur))
            cur = [v, v]
        if c[v] >= 2:
            out.append(tuple(cur))
            out.extend([(v, v)] * (c[v] - 2))
            cur = [v, v]
    if cur is not None:
        out.append(tuple(cur))
    return out


def matrix(records, n, n_script=None):
    """records sorted by (work, fan_ix).  (spans, starts, kept): the spans of at least n words
    as (work, a, b) in span order, the counter as a list of n_script counts, and the kept
    n-grams as (work, start) in span order."""
    if n < 1:
        raise ValueError("ngram must be at least 1")
    if n_script is None:
        n_script = max((o for _, _, o in records), default=-1) + 1
    spans = []
    for run in fan_runs(records):
        for a, b in run_spans(run):      # they close by ascending first word
            if b - a + 1 >= n:
                spans.append((run[0][0], a, b))
    starts = [0] * n_script
    for _, a, b in spans:
        for s in range(a, b - n + 2):
            starts[s] += 1

    def count(s):
        return starts[s] if 0 <= s < n_script else 0
    kept = []
    for w, a, b in spans:
        s = a
        for t in range(a, b - n + 2):
            if count(t) > count(s):
                s = t
        if all(count(t) < count(s) for t in range(s - n + 1, s)) and \
                all(count(t) <= count(s) for t in range(s + 1, s + n)):
            kept.append((w, s))
    return spans, starts, kept


def read_records(path):
    """((work name, fan_ix, orig_ix) in file order) of a match CSV with its header row."""
    with open(path, newline='', encoding='utf-8') as fh:
        return [(r['FAN_WORK_FILENAME'], int(r['FAN_WORK_WORD_INDEX']),
                 int(r['ORIGINAL_SCRIPT_WORD_INDEX'])) for r in csv.DictReader(fh)]


def write_csv(path, records, word=lambda o: "W%d" % o if o % 3 else "w%d" % o):
    """A match CSV of (work name, fan_ix, orig_ix) records, in the order given."""
    with open(path, 'w', newline='', encoding='utf-8') as fh:
        wr = csv.writer(fh)
        wr.writerow(FIELDS)
        for w, f, o in records:
            wr.writerow([w, f, "x", 1, o, word(o), 1, "C", 1, 0.0, 7, 0.0])
