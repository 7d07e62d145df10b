"""Plain-Python restatement of `ao3.py variants`: the two contracts of include/fandom_search.h
(fs_matches_intern, fs_variants) and the two CSVs, written from the issue's text alone.  The
oracle of tests/test_variants_host.py and tests/test_gpu_variants.py."""

import csv
import io

from tests import passages_restated as pr

NONE = 0xFFFFFFFF
MAX_SCRIPT = 1 << 19
CELL_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_CHARACTER',
               'ORIGINAL_SCRIPT_SCENE', 'RANK', 'FAN_WORK_WORD', 'RECORDS', 'WORKS', 'VERBATIM']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_CHARACTER',
               'ORIGINAL_SCRIPT_SCENE', 'RECORDS', 'WORKS', 'SPELLINGS', 'VERBATIM_RECORDS',
               'TOP_FAN_WORD', 'TOP_RECORDS']
CELL_KEYS = ['orig_ix', 'spell', 'n_records', 'n_works']
WORD_KEYS = ['n_records', 'n_spellings', 'n_works', 'first_cell']


def intern(fields):
    """(id, first) of a column's fields (bytes or str, as written): ids in first-appearance
    order, first[k] = the smallest row with spelling k."""
    ids, first, out = {}, [], []
    for r, f in enumerate(fields):
        k = ids.setdefault(f, len(ids))
        if k == len(first):
            first.append(r)
        out.append(k)
    return out, first


def variants(records, n_works, n_script, n_spell):
    """records: (work, orig_ix, spell) in any order.  (words[n_script], cells): dicts with the
    fields of fs_variant_word and fs_variant_cell, the cells in cell order."""
    if len(records) >= 1 << 32 or n_script > MAX_SCRIPT:
        raise NotImplementedError("too many records, or too long a script")
    for w, o, s in records:
        if not (0 <= w < n_works and 0 <= o < n_script and 0 <= s < n_spell):
            raise ValueError("a work, orig_ix or spell out of range")
    by_cell, by_word = {}, {}
    for w, o, s in records:
        by_cell.setdefault((o, s), []).append(w)
        by_word.setdefault(o, []).append(w)
    cells = [dict(orig_ix=o, spell=s, n_records=len(ws), n_works=len(set(ws)))
             for (o, s), ws in by_cell.items()]
    cells.sort(key=lambda c: (c['orig_ix'], -c['n_records'], -c['n_works'], c['spell']))
    words = [dict(n_records=0, n_spellings=0, n_works=0, first_cell=NONE) for _ in range(n_script)]
    for o, ws in by_word.items():
        words[o].update(n_records=len(ws), n_works=len(set(ws)))
    for k, c in enumerate(cells):
        w = words[c['orig_ix']]
        if w['first_cell'] == NONE:
            w['first_cell'] = k
        w['n_spellings'] += 1
    return words, cells


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def variants_csv(text, top=10, min_records=1, fold_case=False):
    """The bytes `ao3.py variants` writes for a match CSV's text: (variants, variants-words)."""
    rows = pr.read_rows(text)
    label, work_of, spell_of, shown, recs = {}, {}, {}, [], []
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        if label.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
        key = r[2].lower() if fold_case else r[2]
        s = spell_of.setdefault(key, len(spell_of))
        if s == len(shown):
            shown.append(r[2])                       # as its first appearance wrote it
        recs.append((work_of.setdefault(r[0], len(work_of)), o, s))
    n_script = max(label) + 1 if label else 0
    words, cells = variants(recs, len(work_of), n_script, len(shown))
    ctab, wtab = [CELL_FIELDS], [WORD_FIELDS]
    for o, w in enumerate(words):
        if not w['n_records']:
            continue
        word, char, scene = label[o]
        mine = cells[w['first_cell']:w['first_cell'] + w['n_spellings']]
        script_key = word.lower() if fold_case else word

        def verbatim(c):
            fan = shown[c['spell']]
            return (fan.lower() if fold_case else fan) == script_key
        wtab.append([o, word, char, scene, w['n_records'], w['n_works'], w['n_spellings'],
                     sum(c['n_records'] for c in mine if verbatim(c)), shown[mine[0]['spell']],
                     mine[0]['n_records']])
        for rank, c in enumerate(mine, 1):
            if (top and rank > top) or c['n_records'] < min_records:
                continue
            ctab.append([o, word, char, scene, rank, shown[c['spell']], c['n_records'],
                         c['n_works'], 1 if verbatim(c) else 0])
    return _csv(ctab), _csv(wtab)
