"""Plain-Python restatement of `ao3.py retellings`: the contract of fs_retellings in
include/fandom_search.h and the two CSVs, written from the issue's text alone, with the join
rule of `passages` restated and the recurrence quadratic as it is stated.  The oracle of
tests/test_retellings_host.py and tests/test_gpu_retellings.py; the product never imports it."""

import csv
import io

NONE = 0xFFFFFFFF
MATCH_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'FAN_WORK_WORD', 'FAN_WORK_ORTH_ID',
                'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_ORTH_ID',
                'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'BEST_MATCH_DISTANCE',
                'BEST_LEVENSHTEIN_DISTANCE', 'BEST_COMBINED_DISTANCE']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'PASSAGES', 'PASSAGE_WORDS', 'CHAIN_PASSAGES', 'CHAIN_WORDS',
               'IN_ORDER_PERCENT', 'DESCENTS', 'ORIGINAL_SCRIPT_WORD_INDEX',
               'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'SCRIPT_SPAN_WORDS', 'CHAIN_SCRIPT_WORDS',
               'FAN_WORK_WORD_INDEX', 'LAST_FAN_WORK_WORD_INDEX', 'SCENES', 'SCENE_SEQUENCE']
PASSAGE_FIELDS = ['FAN_WORK_FILENAME', 'PASSAGE', 'FAN_WORK_WORD_INDEX',
                  'LAST_FAN_WORK_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD_INDEX',
                  'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'WORDS', 'ORIGINAL_SCRIPT_CHARACTER',
                  'ORIGINAL_SCRIPT_SCENE', 'IN_CHAIN', 'CHAIN_POSITION', 'FAN_TEXT', 'SCRIPT_TEXT']
WORK_KEYS = ['n_passages', 'passage_words', 'chain_passages', 'chain_words', 'chain_first',
             'chain_last', 'orig_first', 'orig_last', 'chain_script_words', 'n_descents']
PASSAGE_KEYS = ['first', 'n_words', 'work', 'fan_first', 'fan_last', 'orig_first', 'orig_last',
                'best', 'prev', 'depth', 'chain_pos']


def runs_of(records, max_gap):
    """Lists of record indices: record s continues the run of the record r just before it when
    both are of one work and the fan and the script index each step 1 .. 1 + max_gap ahead."""
    runs = []
    for i, s in enumerate(records):
        if i:
            r = records[i - 1]
            if (s[0], s[1]) < (r[0], r[1]):
                raise ValueError("records out of (work, fan_ix) order at %d" % i)
            if s[0] == r[0] and 1 <= s[1] - r[1] <= 1 + max_gap and 1 <= s[2] - r[2] <= 1 + max_gap:
                runs[-1].append(i)
                continue
        runs.append([i])
    return runs


def retellings(records, n_works, min_words=6, max_gap=0):
    """records: (work, fan_ix, orig_ix) sorted by (work, fan_ix).  (works, passages): dicts with
    the fields of fs_retelling, one per work, and of fs_retelling_passage, in record order."""
    if min_words == 0:
        raise ValueError("min_words must be at least 1")
    if len(records) >= 1 << 32:
        raise NotImplementedError("too many records")
    for w, _, _ in records:
        if not 0 <= w < n_works:
            raise ValueError("a work out of range")
    found = []
    for run in runs_of(records, max_gap):
        if len(run) < min_words:
            continue
        a, b = records[run[0]], records[run[-1]]
        found.append(dict(first=run[0], n_words=len(run), work=a[0], fan_first=a[1], fan_last=b[1],
                          orig_first=a[2], orig_last=b[2], best=0, prev=NONE, depth=0,
                          chain_pos=0))
    works = [dict(n_passages=0, passage_words=0, chain_passages=0, chain_words=0,
                  chain_first=NONE, chain_last=NONE, orig_first=0, orig_last=0,
                  chain_script_words=0, n_descents=0) for _ in range(n_works)]
    by_work = {}
    for k, p in enumerate(found):
        by_work.setdefault(p['work'], []).append(k)
    for w, mine in by_work.items():
        for x, i in enumerate(mine):
            p = found[i]
            top, prev = 0, NONE
            for j in mine[:x]:
                q = found[j]
                if p['orig_first'] > q['orig_last'] and q['best'] > top:   # the smallest j on a tie
                    top, prev = q['best'], j
            p['best'] = p['n_words'] + top
            p['prev'] = prev
            p['depth'] = 1 if prev == NONE else 1 + found[prev]['depth']
        end = mine[0]
        for i in mine:
            if found[i]['best'] > found[end]['best']:                      # the smallest i on a tie
                end = i
        chain, i = [], end
        while i != NONE:
            chain.append(i)
            i = found[i]['prev']
        chain.reverse()
        for at, i in enumerate(chain, 1):
            found[i]['chain_pos'] = at
            assert found[i]['depth'] == at
        works[w] = dict(
            n_passages=len(mine), passage_words=sum(found[i]['n_words'] for i in mine),
            chain_passages=len(chain), chain_words=found[end]['best'], chain_first=chain[0],
            chain_last=end, orig_first=found[chain[0]]['orig_first'],
            orig_last=found[end]['orig_last'],
            chain_script_words=sum(found[i]['orig_last'] - found[i]['orig_first'] + 1
                                   for i in chain),
            n_descents=sum(1 for a, b in zip(mine, mine[1:])
                           if found[b]['orig_first'] <= found[a]['orig_last']))
        assert found[end]['best'] == sum(found[i]['n_words'] for i in chain)
        assert (works[w]['n_descents'] == 0) == (len(chain) == len(mine))
    return works, found


def read_rows(text):
    """Text rows of a match CSV (dated file with header, or batch file without)."""
    rows = [r for r in csv.reader(io.StringIO(text, newline='')) if r]
    if rows and rows[0] == MATCH_FIELDS:
        rows = rows[1:]
    return rows


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def retellings_csv(text, min_words=6, max_gap=0, min_passages=2, min_share=0):
    """The bytes `ao3.py retellings` writes for a match CSV's text: (retellings,
    retellings-passages)."""
    rows = read_rows(text)
    label, work_of, keyed = {}, {}, []
    for k, r in enumerate(rows):
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        have = label.setdefault(o, lab)
        if have != lab:
            what = next(n for n, x, y in zip(('word', 'character', 'scene'), have, lab) if x != y)
            raise ValueError("script word %d has two %ss" % (o, what))
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    srt = [rows[k] for _, _, k in keyed]
    recs = [(w, f, int(rows[k][4])) for w, f, k in keyed]
    works, found = retellings(recs, len(work_of), min_words, max_gap)
    names = list(work_of)
    listed = [w for w, r in enumerate(works)
              if r['n_passages'] and r['chain_passages'] >= min_passages
              and r['chain_words'] * 100 // r['passage_words'] >= min_share]
    listed.sort(key=lambda w: (-works[w]['chain_words'], -works[w]['chain_passages']))   # stable
    wtab, ptab = [WORK_FIELDS], [PASSAGE_FIELDS]
    for w in listed:
        r = works[w]
        mine = [p for p in found if p['work'] == w]
        chain = sorted((p for p in mine if p['chain_pos']), key=lambda p: p['chain_pos'])
        scenes = [srt[p['first']][8] for p in chain]
        seq = [s for i, s in enumerate(scenes) if i == 0 or scenes[i - 1] != s]
        wtab.append([names[w], r['n_passages'], r['passage_words'], r['chain_passages'],
                     r['chain_words'], r['chain_words'] * 100 // r['passage_words'],
                     r['n_descents'], r['orig_first'], r['orig_last'],
                     r['orig_last'] - r['orig_first'] + 1, r['chain_script_words'],
                     chain[0]['fan_first'], chain[-1]['fan_last'], len(set(scenes)),
                     ' > '.join(seq)])
        for k, p in enumerate(mine, 1):
            part = srt[p['first']:p['first'] + p['n_words']]
            ptab.append([names[w], k, p['fan_first'], p['fan_last'], p['orig_first'],
                         p['orig_last'], p['n_words'], part[0][7], part[0][8],
                         1 if p['chain_pos'] else 0, p['chain_pos'] or '',
                         ' '.join(x[2] for x in part), ' '.join(x[5] for x in part)])
    return _csv(wtab), _csv(ptab)
