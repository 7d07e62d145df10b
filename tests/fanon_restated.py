"""Plain-Python restatement of `ao3.py fanon`: the contract of fs_fanon in
include/fandom_search.h and the four CSVs, written from the issue's text alone: dicts keyed by
tuples, one loop per definition.  The oracle of tests/test_fanon_host.py and
tests/test_gpu_fanon.py and the writer of the golden files; the product never imports it, and
it shares no code with fandom_search_amd/fanon.py."""

import csv
import io
import os

NO_ID = 0xFFFFFFFF
WORK_KEYS = ['n_tokens', 'n_positions', 'shared_positions', 'canon_positions',
             'common_positions', 'n_passages', 'shared_tokens', 'canon_tokens', 'longest_start',
             'longest_tokens']
GRAM_KEYS = ['work', 'start', 'works', 'occurrences']
PASSAGE_KEYS = ['work', 'start', 'n_tokens', 'phrase', 'least', 'most']
PHRASE_KEYS = ['work', 'start', 'n_tokens', 'n_passages', 'n_works', 'least', 'most', 'reserved']
PHRASE_FIELDS = ['RANK', 'TOKENS', 'WORKS', 'PASSAGES', 'LEAST_GRAM_WORKS', 'MOST_GRAM_WORKS',
                 'FIRST_FAN_WORK_FILENAME', 'FIRST_FAN_WORK_WORD_INDEX', 'TEXT']
PASSAGE_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'LAST_FAN_WORK_WORD_INDEX', 'TOKENS',
                  'PHRASE', 'LEAST_GRAM_WORKS', 'MOST_GRAM_WORKS', 'TEXT']
GRAM_FIELDS = ['RANK', 'WORKS', 'OCCURRENCES', 'FIRST_FAN_WORK_FILENAME',
               'FIRST_FAN_WORK_WORD_INDEX', 'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'TOKENS', 'POSITIONS', 'SHARED_POSITIONS', 'CANON_POSITIONS',
               'COMMON_POSITIONS', 'PASSAGES', 'SHARED_TOKENS', 'CANON_TOKENS',
               'LONGEST_FAN_WORK_WORD_INDEX', 'LONGEST_TOKENS', 'LONGEST_TEXT']


def fanon(works, scripts, k=8, min_works=2, max_share=100):
    """works: a list of id lists; scripts: a list of id lists (NO_ID for a word that is no fan
    token).  (works, grams, passages, phrases, totals): lists of dicts with the fields of the
    four records in output order, and {'positions', 'distinct'}."""
    if not 2 <= k <= 32 or min_works < 1 or not 1 <= max_share <= 100:
        raise ValueError("k, min_works or max_share out of range")
    n_works = len(works)
    # grams
    occurrences, in_works, first = {}, {}, {}
    for w, ids in enumerate(works):
        for p in range(len(ids) - k + 1):
            g = tuple(ids[p:p + k])
            occurrences[g] = occurrences.get(g, 0) + 1
            in_works.setdefault(g, set()).add(w)
            first.setdefault(g, (w, p))
    # canon
    canon = set()
    for ids in scripts:
        for p in range(len(ids) - k + 1):
            g = tuple(ids[p:p + k])
            if NO_ID not in g:
                canon.add(g)

    def n_in(g):
        return len(in_works[g])

    def is_common(g):
        return n_in(g) * 100 > max_share * n_works

    def is_shared(g):
        return n_in(g) >= min_works and g not in canon and not is_common(g)
    grams = [{'work': first[g][0], 'start': first[g][1], 'works': n_in(g),
              'occurrences': occurrences[g]}
             for g in sorted((g for g in first if is_shared(g)), key=lambda g: first[g])]
    # passages
    passages, sequences, records = [], [], []
    for w, ids in enumerate(works):
        L = len(ids)
        n_pos = max(0, L - k + 1)
        flags = [tuple(ids[p:p + k]) for p in range(n_pos)]
        shared = [is_shared(g) for g in flags]
        mine = []
        p = 0
        while p < n_pos:
            if not shared[p]:
                p += 1
                continue
            q = p
            while q + 1 < n_pos and shared[q + 1]:
                q += 1
            counts = [n_in(flags[j]) for j in range(p, q + 1)]
            mine.append({'work': w, 'start': p, 'n_tokens': q - p + k, 'phrase': None,
                         'least': min(counts), 'most': max(counts)})
            sequences.append(tuple(ids[p:q + k]))
            p = q + 1
        passages += mine
        shared_tokens, canon_tokens = set(), set()
        for p in range(n_pos):
            if shared[p]:
                shared_tokens.update(range(p, p + k))
            if flags[p] in canon:
                canon_tokens.update(range(p, p + k))
        longest = None
        for m in mine:
            if longest is None or m['n_tokens'] > longest['n_tokens']:
                longest = m
        records.append({'n_tokens': L, 'n_positions': n_pos, 'shared_positions': sum(shared),
                        'canon_positions': sum(1 for g in flags if g in canon),
                        'common_positions': sum(1 for g in flags if is_common(g)),
                        'n_passages': len(mine), 'shared_tokens': len(shared_tokens),
                        'canon_tokens': len(canon_tokens),
                        'longest_start': longest['start'] if longest else 0,
                        'longest_tokens': longest['n_tokens'] if longest else 0})
    # phrases
    by_sequence = {}
    for j, seq in enumerate(sequences):
        by_sequence.setdefault(seq, []).append(j)
    order = sorted(by_sequence, key=lambda seq: by_sequence[seq][0])
    phrases = []
    for r, seq in enumerate(order):
        members = [passages[j] for j in by_sequence[seq]]
        for m in members:
            m['phrase'] = r
        assert len({(m['least'], m['most']) for m in members}) == 1
        phrases.append({'work': members[0]['work'], 'start': members[0]['start'],
                        'n_tokens': len(seq), 'n_passages': len(members),
                        'n_works': len({m['work'] for m in members}),
                        'least': members[0]['least'], 'most': members[0]['most'], 'reserved': 0})
    totals = {'positions': sum(r['n_positions'] for r in records), 'distinct': len(first)}
    return records, grams, passages, phrases, totals


def corpus(directory, scripts=(), keep_case=False, num_works=-1, skip_works=0, listing=None):
    """(names, texts per work, id lists per work, id lists per script) of a directory of fan
    works and script markups, as the command reads them."""
    from fandom_search_amd import search
    names = search.list_fan_works(directory, skip_works, num_works, listing)
    texts = [search.read_work_tokens(f) for f in names]
    ids = {}
    works = []
    for toks in texts:
        works.append([ids.setdefault(t if keep_case else t.lower(), len(ids)) for t in toks])
    canon = []
    for s in scripts:
        rows = search.load_markup_script(s)[1:]
        canon.append([ids.get(r[0] if keep_case else r[0].lower(), NO_ID) for r in rows])
    return names, texts, works, canon


def tables(directory, scripts=(), length=8, min_works=2, max_share=100, keep_case=False,
           top=1000, num_works=-1, skip_works=0, listing=None):
    """The rows of the four CSVs, without headers: phrases, passages, grams, works."""
    names, texts, works, canon = corpus(directory, scripts, keep_case, num_works, skip_works,
                                        listing)
    records, grams, passages, phrases, _ = fanon(works, canon, length, min_works, max_share)

    def text(w, p, n):
        return ' '.join(texts[w][p:p + n])
    ranked = sorted(range(len(phrases)),
                    key=lambda j: (-phrases[j]['n_works'], -phrases[j]['most'],
                                   -phrases[j]['n_tokens'], j))
    if top:
        ranked = ranked[:top]
    rank_of = {j: r + 1 for r, j in enumerate(ranked)}
    t_phrases = []
    for j in ranked:
        f = phrases[j]
        t_phrases.append([rank_of[j], f['n_tokens'], f['n_works'], f['n_passages'], f['least'],
                          f['most'], names[f['work']], f['start'],
                          text(f['work'], f['start'], f['n_tokens'])])
    t_passages = [[names[p['work']], p['start'], p['start'] + p['n_tokens'] - 1, p['n_tokens'],
                   rank_of.get(p['phrase'], ''), p['least'], p['most'],
                   text(p['work'], p['start'], p['n_tokens'])] for p in passages]
    g_ranked = sorted(range(len(grams)),
                      key=lambda j: (-grams[j]['works'], -grams[j]['occurrences'], j))
    if top:
        g_ranked = g_ranked[:top]
    t_grams = [[r + 1, grams[j]['works'], grams[j]['occurrences'], names[grams[j]['work']],
                grams[j]['start'], text(grams[j]['work'], grams[j]['start'], length)]
               for r, j in enumerate(g_ranked)]
    t_works = [[names[w], r['n_tokens'], r['n_positions'], r['shared_positions'],
                r['canon_positions'], r['common_positions'], r['n_passages'], r['shared_tokens'],
                r['canon_tokens'], r['longest_start'] if r['n_passages'] else '',
                r['longest_tokens'], text(w, r['longest_start'], r['longest_tokens'])]
               for w, r in enumerate(records)]
    return t_phrases, t_passages, t_grams, t_works


HEADS = (PHRASE_FIELDS, PASSAGE_FIELDS, GRAM_FIELDS, WORK_FIELDS)
SUFFIXES = ('-fanon.csv', '-fanon-passages.csv', '-fanon-grams.csv', '-fanon-works.csv')


def csv_text(head, rows):
    out = io.StringIO(newline='')
    w = csv.writer(out)
    w.writerow(head)
    w.writerows(rows)
    return out.getvalue()


def read_csv(path):
    with open(path, newline='', encoding='utf-8') as fh:
        return fh.read()


def default_prefix(directory):
    return os.path.basename(os.path.normpath(directory))
