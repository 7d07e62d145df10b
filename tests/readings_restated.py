"""Plain-Python restatement of `ao3.py readings`: the contract of fs_readings in
include/fandom_search.h and the two CSVs, written from the issue's text alone.  The oracle of
tests/test_readings_host.py and tests/test_gpu_readings.py; the product never imports it."""

import csv
import io

from tests import passages_restated as pr

MAX_SCRIPT = 1 << 19
READING_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'WORDS',
                  'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'RANK', 'PASSAGES',
                  'WORKS', 'CHANGED_WORDS', 'VERBATIM', 'FIRST_FAN_WORK_FILENAME', 'FAN_TEXT',
                  'SCRIPT_TEXT']
SPAN_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'WORDS',
               'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'PASSAGES', 'WORKS',
               'READINGS', 'VERBATIM_PASSAGES', 'TOP_FAN_TEXT', 'TOP_WORKS', 'SCRIPT_TEXT']
READING_KEYS = ['first', 'orig_first', 'orig_last', 'n_words', 'n_passages', 'n_works', 'span',
                'rank', 'reserved']
SPAN_KEYS = ['orig_first', 'orig_last', 'n_passages', 'n_works', 'n_readings', 'first_reading']
UNKNOWN_WORD = '[?]'


def readings(records, n_works, n_script, n_spell, min_words=6, max_gap=0):
    """records: (work, fan_ix, orig_ix, spell) sorted by (work, fan_ix).  (readings, spans,
    n_passages): dicts with the fields of fs_reading and fs_reading_span, in output order."""
    if min_words == 0:
        raise ValueError("min_words must be at least 1")
    if len(records) >= 1 << 32 or n_script > MAX_SCRIPT:
        raise NotImplementedError("too many records, or too long a script")
    for w, _, o, s in records:
        if not (0 <= w < n_works and 0 <= o < n_script and 0 <= s < n_spell):
            raise ValueError("a work, orig_ix or spell out of range")
    found = pr.passages([(w, f, o, 0.0, 0.0) for w, f, o, _ in records], min_words, max_gap)
    by_reading = {}
    for p in found:
        recs = records[p['first']:p['first'] + p['n_words']]
        o0 = recs[0][2]
        key = (o0, tuple((r[2] - o0, r[3]) for r in recs))
        by_reading.setdefault(key, []).append((p['first'], recs[0][0], recs[-1][2]))
    by_span = {}
    for (o0, seq), ps in by_reading.items():
        span = (o0, ps[0][2])
        assert all(p[2] == span[1] for p in ps)
        by_span.setdefault(span, []).append(
            dict(first=ps[0][0], orig_first=span[0], orig_last=span[1], n_words=len(seq),
                 n_passages=len(ps), n_works=len({p[1] for p in ps}), reserved=0,
                 works={p[1] for p in ps}))
    out_r, out_s = [], []
    for span in sorted(by_span):
        mine = sorted(by_span[span], key=lambda r: (-r['n_works'], -r['n_passages'], r['first']))
        works = set()
        for rank, r in enumerate(mine, 1):
            works |= r.pop('works')
            r.update(span=len(out_s), rank=rank)
        out_s.append(dict(orig_first=span[0], orig_last=span[1],
                          n_passages=sum(r['n_passages'] for r in mine), n_works=len(works),
                          n_readings=len(mine), first_reading=len(out_r)))
        out_r += mine
    return out_r, out_s, len(found)


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def readings_csv(text, min_words=6, max_gap=0, top=10, min_works=1, fold_case=False):
    """The bytes `ao3.py readings` writes for a match CSV's text: (readings, readings-spans)."""
    rows = pr.read_rows(text)

    def fold(t):
        return t.lower() if fold_case else t
    label, work_of, spell_of, keyed = {}, {}, {}, []
    for k, r in enumerate(rows):
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        have = label.setdefault(o, lab)
        if have != lab:
            what = next(n for n, x, y in zip(('word', 'character', 'scene'), have, lab) if x != y)
            raise ValueError("script word %d has two %ss" % (o, what))
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
        spell_of.setdefault(fold(r[2]), len(spell_of))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    srt = [rows[k] for _, _, k in keyed]
    recs = [(w, f, int(rows[k][4]), spell_of[fold(rows[k][2])]) for w, f, k in keyed]
    n_script = max(label) + 1 if label else 0
    found, spans, _ = readings(recs, len(work_of), n_script, len(spell_of), min_words, max_gap)
    names = list(work_of)
    rtab, stab = [READING_FIELDS], [SPAN_FIELDS]
    for s in spans:
        a, b = s['orig_first'], s['orig_last']
        _, char, scene = label[a]
        mine = found[s['first_reading']:s['first_reading'] + s['n_readings']]
        lines = []
        for r in mine:
            part = srt[r['first']:r['first'] + r['n_words']]
            changed = sum(1 for p in part if fold(p[2]) != fold(p[5]))
            lines.append((changed, ' '.join(p[2] for p in part), ' '.join(p[5] for p in part),
                          part[0][0]))
        stab.append([a, b, b - a + 1, char, scene, s['n_passages'], s['n_works'], s['n_readings'],
                     sum(r['n_passages'] for r, l in zip(mine, lines) if l[0] == 0),
                     lines[0][1], mine[0]['n_works'],
                     ' '.join(label[o][0] if o in label else UNKNOWN_WORD for o in range(a, b + 1))])
        for r, (changed, fan_text, script_text, name) in zip(mine, lines):
            if (top and r['rank'] > top) or r['n_works'] < min_works:
                continue
            assert name == names[recs[r['first']][0]]
            rtab.append([a, b, r['n_words'], char, scene, r['rank'], r['n_passages'],
                         r['n_works'], changed, 1 if changed == 0 else 0, name, fan_text,
                         script_text])
    return _csv(rtab), _csv(stab)
