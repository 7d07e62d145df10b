"""Plain-Python restatement of `ao3.py alignments`: the contract of fs_alignments in
include/fandom_search.h and the two CSVs, record by record, the look-back quadratic as the
rule states it.  The oracle of tests/test_alignments_host.py and tests/test_gpu_alignments.py
and of the committed tests/golden/alignments_lines.*.csv; the product never imports it."""

import csv
import io
import math

MATCH_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'FAN_WORK_WORD', 'FAN_WORK_ORTH_ID',
                'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_ORTH_ID',
                'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'BEST_MATCH_DISTANCE',
                'BEST_LEVENSHTEIN_DISTANCE', 'BEST_COMBINED_DISTANCE']
ALIGNMENT_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_START', 'FAN_WORK_WORD_END',
                    'ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'MATCHED_WORDS',
                    'EXACT_WORDS', 'SCORE', 'FAN_WORDS_SKIPPED', 'SCRIPT_WORDS_SKIPPED', 'PIECES',
                    'SIDE_RECORDS', 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE',
                    'MEAN_COMBINED_DISTANCE', 'MAX_COMBINED_DISTANCE', 'FAN_WORK_TEXT',
                    'ORIGINAL_SCRIPT_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'ALIGNMENTS', 'ALIGNED_WORDS', 'LONGEST', 'FAN_WORDS_SKIPPED',
               'SCRIPT_WORDS_SKIPPED', 'PASSAGE_WORDS', 'GAINED_WORDS']
KEYS = ['first', 'last', 'n_words', 'n_exact', 'score', 'fan_skipped', 'orig_skipped', 'pieces',
        'tree_records', 'reserved', 'path_at']


def check(n_rows, min_words, reach, match, gap):
    """The argument rules of fs_alignments: ValueError where it answers FS_E_INVALID,
    NotImplementedError where FS_E_UNSUPPORTED."""
    if min_words < 1 or match < 1 or reach > 63 or match > 16 or gap > 16 or reach < 0 or gap < 0:
        raise ValueError("min_words and match at least 1, reach 0 to 63, gap 0 to 16, match at "
                         "most 16")
    if n_rows >= 1 << 32 or n_rows * match >= 1 << 32:
        raise NotImplementedError("too many records")


def chain(records, reach=4, match=2, gap=1):
    """(best, prev) per record of records (work, fan_ix, orig_ix, ...) sorted by (work, fan_ix);
    prev is None for a root."""
    best, prev = [], []
    for i, s in enumerate(records):
        if i:
            r = records[i - 1]
            if (s[0], s[1]) < (r[0], r[1]):
                raise ValueError("records out of (work, fan_ix) order at %d" % i)
        top, at = 0, None
        for j in range(i - 1, -1, -1):                 # the nearest record first
            q = records[j]
            df, do = s[1] - q[1], s[2] - q[2]
            if q[0] != s[0] or df > reach + 1:         # sorted: nothing in front of j is nearer
                break
            if not (1 <= df and 1 <= do <= reach + 1):
                continue
            value = best[j] - gap * ((df - 1) + (do - 1))
            if value > top:                            # the largest j on a tie: it came first
                top, at = value, j
        best.append(match + top)
        prev.append(at)
    return best, prev


def alignments(records, min_words=6, reach=4, match=2, gap=1):
    """records: (work, fan_ix, orig_ix, comb) sorted by (work, fan_ix).  (alignments, path):
    dicts with the fields of fs_alignment in root order, and the record indices of their paths,
    path after path."""
    check(len(records), min_words, reach, match, gap)
    best, prev = chain(records, reach, match, gap)
    root = []
    for i, p in enumerate(prev):
        root.append(i if p is None else root[p])
    trees = {}
    for i, r in enumerate(root):
        trees.setdefault(r, []).append(i)
    found, path = [], []
    for r in sorted(trees):
        mine = trees[r]
        peak = mine[0]
        for i in mine:
            if best[i] > best[peak]:                   # the smallest i on a tie
                peak = i
        walk, i = [], peak
        while i is not None:
            walk.append(i)
            i = prev[i]
        walk.reverse()
        assert walk[0] == r
        if len(walk) < min_words:
            continue
        steps = [(records[b][1] - records[a][1], records[b][2] - records[a][2])
                 for a, b in zip(walk, walk[1:])]
        found.append(dict(
            first=r, last=peak, n_words=len(walk),
            n_exact=sum(1 for i in walk if records[i][3] <= 0), score=best[peak],
            fan_skipped=sum(df - 1 for df, _ in steps),
            orig_skipped=sum(do - 1 for _, do in steps),
            pieces=1 + sum(1 for df, do in steps if df != 1 or do != 1),
            tree_records=len(mine), reserved=0, path_at=len(path)))
        assert best[peak] == match * len(walk) - gap * (found[-1]['fan_skipped']
                                                        + found[-1]['orig_skipped'])
        path.extend(walk)
    return found, path


def passage_words(records, min_words):
    """{work: the records inside its passages} under the join of `passages` at max_gap 0."""
    runs = []
    for i, s in enumerate(records):
        if i:
            r = records[i - 1]
            if s[0] == r[0] and s[1] - r[1] == 1 and s[2] - r[2] == 1:
                runs[-1].append(i)
                continue
        runs.append([i])
    words = {}
    for run in runs:
        if len(run) >= min_words:
            w = records[run[0]][0]
            words[w] = words.get(w, 0) + len(run)
    return words


def _max(values):
    best = float('nan')
    for v in values:
        if math.isnan(v):
            continue
        if math.isnan(best) or v > best:
            best = v
    return best


def read_rows(text):
    """Text rows of a match CSV (dated file with header, or batch file without)."""
    rows = [r for r in csv.reader(io.StringIO(text, newline='')) if r]
    if rows and rows[0] == MATCH_FIELDS:
        rows = rows[1:]
    return rows


def _num(text):
    return float(text) if text != '' else float('nan')


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def _text(words, skips):
    """The words joined by a space, [+k] where the link between two of them skips k words."""
    out = [words[0]]
    for word, k in zip(words[1:], skips):
        if k:
            out.append('[+%d]' % k)
        out.append(word)
    return ' '.join(out)


def alignments_csv(text, min_words=6, reach=4, match=2, gap=1):
    """The bytes `ao3.py alignments` writes for a match CSV's text: (alignments,
    alignments-works)."""
    rows = read_rows(text)
    work_of, keyed = {}, []
    for k, r in enumerate(rows):
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    srt = [rows[k] for _, _, k in keyed]
    recs = [(w, f, int(rows[k][4]), _num(rows[k][11])) for w, f, k in keyed]
    found, path = alignments(recs, min_words, reach, match, gap)
    names = list(work_of)
    atab, per = [ALIGNMENT_FIELDS], {}
    for a in found:
        walk = path[a['path_at']:a['path_at'] + a['n_words']]
        head, tail = recs[walk[0]], recs[walk[-1]]
        combs = [recs[i][3] for i in walk]
        atab.append([names[head[0]], head[1], tail[1], head[2], tail[2], a['n_words'],
                     a['n_exact'], a['score'], a['fan_skipped'], a['orig_skipped'], a['pieces'],
                     a['tree_records'] - a['n_words'], srt[walk[0]][7], srt[walk[0]][8],
                     sum(combs, 0.0) / len(combs), _max(combs),
                     _text([srt[i][2] for i in walk],
                           [recs[b][1] - recs[a_][1] - 1 for a_, b in zip(walk, walk[1:])]),
                     _text([srt[i][5] for i in walk],
                           [recs[b][2] - recs[a_][2] - 1 for a_, b in zip(walk, walk[1:])])])
        w = per.setdefault(head[0], [0, 0, 0, 0, 0])
        w[0] += 1
        w[1] += a['n_words']
        w[2] = max(w[2], a['n_words'])
        w[3] += a['fan_skipped']
        w[4] += a['orig_skipped']
    joined = passage_words(recs, min_words)
    wtab = [WORK_FIELDS]
    for w in sorted(per):
        n, words, longest, fsk, osk = per[w]
        wtab.append([names[w], n, words, longest, fsk, osk, joined.get(w, 0),
                     words - joined.get(w, 0)])
    return _csv(atab), _csv(wtab)
