"""`ao3.py readings`: the wordings fans give each quoted stretch of the script.

`passages` lists every reused span of every fan work; `variants` says what fans wrote at one
script word.  This command collates whole passages: two passages are the same reading when
they start at the same script word and their records step over the same script offsets with
the same fan spellings.  Per reading its passages and the distinct works behind them, the
readings of a span (first and last script word) ranked by works, then passages, then first
appearance; and per span its passages, works, readings, how many passages are verbatim and
its top reading.

The records are sorted by (work, FAN_WORK_WORD_INDEX) as `passages` sorts them, the spelling
ids along with them.  The fan words are numbered in first-appearance order: on the device
(fs_matches_intern over the file's bytes) or, under the python reader, by a dict over the rows.
The passages, the grouping, the distinct counts and the ranking come from the GPU
(fs_readings); reading labels and writing the CSVs is host plumbing, and only the records of
each reading's first passage are decoded to text.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import _FAN_WORD, sort_records
from .quotes import UNKNOWN_WORD, word_labels
from .variants import fold_key, merge_spellings

READING_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'WORDS',
                  'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'RANK', 'PASSAGES',
                  'WORKS', 'CHANGED_WORDS', 'VERBATIM', 'FIRST_FAN_WORK_FILENAME', 'FAN_TEXT',
                  'SCRIPT_TEXT']
SPAN_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'WORDS',
               'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'PASSAGES', 'WORKS',
               'READINGS', 'VERBATIM_PASSAGES', 'TOP_FAN_TEXT', 'TOP_WORKS', 'SCRIPT_TEXT']


def find_readings(work, fan_ix, orig_ix, spell, n_works, n_script, n_spell, min_words=6,
                  max_gap=0, device=0):
    """(abi.READING_DTYPE readings in span and rank order, abi.READING_SPAN_DTYPE spans in
    script order, passages) of records sorted by (work, fan_ix)."""
    work, fan, orig, spell = (abi.as_u32(v) for v in (work, fan_ix, orig_ix, spell))
    n = len(work)
    if not (len(fan) == len(orig) == len(spell) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    cap = n // max(1, int(min_words)) + 1               # passages never outnumber this
    got_p = C.c_uint64(0)
    readings, spans = grow(lambda r, cap_r, got_r, s, cap_s, got_s: L.fs_readings(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(spell, C.c_uint32), n, int(n_works), int(n_script),
        int(n_spell), int(min_words), int(max_gap), r, cap_r, s, cap_s, got_r, got_s,
        C.byref(got_p)), [abi.READING_DTYPE, abi.READING_SPAN_DTYPE], [cap, cap], "fs_readings")
    return readings, spans, int(got_p.value)


def tables(rows, min_words=6, max_gap=0, top=10, min_works=1, fold_case=False, device=0):
    """(readings, spans): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    order, work, fan, orig, _, _ = sort_records(rows)
    spell, _, shown = merge_spellings([r[_FAN_WORD] for r in rows], fold_case)

    def fan_words(recs):
        return [rows[i][_FAN_WORD] for i in recs]
    return _tables(labels, work_names(rows), fan_words, order, work, fan, orig, spell[order],
                   n_script_of(orig), len(shown), min_words, max_gap, top, min_works, fold_case,
                   device)


def tables_device(mf, min_words=6, max_gap=0, top=10, min_works=1, fold_case=False, device=0):
    """tables over a matches.MatchFile: the fan words numbered on the device, one text decoded
    per spelling, three labels per script word and the fan words of each reading's first
    passage; None when a script word's records spell a label in two ways (tables() then
    decides)."""
    order, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    raw, first = mf.intern(_FAN_WORD)
    remap, _, shown = merge_spellings(mf.text(_FAN_WORD, first), fold_case)
    spell = np.take(remap, raw)[order] if mf.n else np.zeros(0, dtype=np.uint32)

    def fan_words(recs):
        return mf.text(_FAN_WORD, recs)
    return _tables(labels, mf.names, fan_words, order, work, fan, orig, spell, n_script,
                   len(shown), min_words, max_gap, top, min_works, fold_case, device)


def _tables(labels, names, fan_words, order, work, fan, orig, spell, n_script, n_spell,
            min_words, max_gap, top, min_works, fold_case, device):
    readings, spans, _ = find_readings(work, fan, orig, spell, len(names), n_script, n_spell,
                                       min_words, max_gap, device)
    # the records of every reading's first passage, reading after reading
    first = readings['first'].astype(np.int64)
    count = readings['n_words'].astype(np.int64)
    ends = np.cumsum(count)
    pos = np.repeat(first - (ends - count), count) + np.arange(ends[-1] if len(ends) else 0)
    fans = fan_words(order[pos])
    origs = orig[pos].tolist()
    unknown = (UNKNOWN_WORD, '', '')
    rtab, stab, lines = [], [], []
    for j, r in enumerate(readings):
        lo, hi = int(ends[j]) - int(count[j]), int(ends[j])
        script = [labels[o][0] for o in origs[lo:hi]]
        changed = sum(1 for f, s in zip(fans[lo:hi], script)
                      if fold_key(f, fold_case) != fold_key(s, fold_case))
        lines.append((changed, ' '.join(fans[lo:hi]), ' '.join(script)))
    for s in spans:
        a, b = int(s['orig_first']), int(s['orig_last'])
        _, char, scene = labels[a]                  # a span starts at a record
        r0, k = int(s['first_reading']), int(s['n_readings'])
        verbatim = sum(int(readings[j]['n_passages']) for j in range(r0, r0 + k)
                       if lines[j][0] == 0)
        stab.append([a, b, b - a + 1, char, scene, int(s['n_passages']), int(s['n_works']), k,
                     verbatim, lines[r0][1], int(readings[r0]['n_works']),
                     ' '.join(labels.get(o, unknown)[0] for o in range(a, b + 1))])
        for j in range(r0, r0 + (min(k, top) if top else k)):
            r = readings[j]
            if int(r['n_works']) < min_works:
                continue
            changed, fan_text, script_text = lines[j]
            rtab.append([a, b, int(r['n_words']), char, scene, int(r['rank']),
                         int(r['n_passages']), int(r['n_works']), changed,
                         1 if changed == 0 else 0, names[int(work[int(r['first'])])], fan_text,
                         script_text])
    return rtab, stab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-readings.csv', '-readings-spans.csv'))


def process(args):
    """`ao3.py readings matches [-o PREFIX] [--min-words M] [--max-gap G] [--top K]
    [--min-works W] [--fold-case] [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.top, args.min_works, args.fold_case, args.device)
    return run(args, (READING_FIELDS, SPAN_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
