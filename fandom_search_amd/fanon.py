"""`ao3.py fanon`: the phrases fan works share with each other and the script lacks.

Every other analysis command starts from the match csv and sees a fan work only where it
touches the script.  This one reads the fan works themselves: a gram is K consecutive tokens
of one work; it is canon when a script holds the same K words in a row, common when more than
--max-share percent of the works hold it, and shared when at least --min-works works hold it
and it is neither.  A maximal run of shared positions in a work is a passage, equal passages
are one phrase.  Reposts, memes, copied disclaimers and lines of famous fics surface as
phrases; the per-work figures say how much of a work is somebody else's words.

The works are those `search` lists for the same directory, -n, -s and --listing, and a token's
index is the FAN_WORK_WORD_INDEX of the match csv.  The host reads and tokenises the works
(through a pool of processes where search.default_workers() gives one), folds the texts and
numbers them; the grams, flags, passages, phrases and per-work figures come from the GPU
(fs_fanon), which sees ids only.  Ranking is a stable host sort of one key per row, and only
the tokens an output row shows are decoded.  No vector table is involved.
"""

import os

import numpy as np

from . import abi
from .command import write_tables

PHRASE_FIELDS = ['RANK', 'TOKENS', 'WORKS', 'PASSAGES', 'LEAST_GRAM_WORKS', 'MOST_GRAM_WORKS',
                 'FIRST_FAN_WORK_FILENAME', 'FIRST_FAN_WORK_WORD_INDEX', 'TEXT']
PASSAGE_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'LAST_FAN_WORK_WORD_INDEX', 'TOKENS',
                  'PHRASE', 'LEAST_GRAM_WORKS', 'MOST_GRAM_WORKS', 'TEXT']
GRAM_FIELDS = ['RANK', 'WORKS', 'OCCURRENCES', 'FIRST_FAN_WORK_FILENAME',
               'FIRST_FAN_WORK_WORD_INDEX', 'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'TOKENS', 'POSITIONS', 'SHARED_POSITIONS', 'CANON_POSITIONS',
               'COMMON_POSITIONS', 'PASSAGES', 'SHARED_TOKENS', 'CANON_TOKENS',
               'LONGEST_FAN_WORK_WORD_INDEX', 'LONGEST_TOKENS', 'LONGEST_TEXT']
CHUNK = 31                    # works a pool job reads (the chunk size of search's pool)


def _read_chunk(filenames):
    """What a pool worker does with a chunk of works: token counts per work, the chunk's
    tokens as indices into the chunk's distinct texts, and those texts -- 4 bytes per token on
    the way back instead of one string."""
    from . import search
    lens = np.zeros(len(filenames), dtype=np.int64)
    flat = []
    for i, f in enumerate(filenames):
        toks = search.read_work_tokens(f)
        lens[i] = len(toks)
        flat += toks
    codes, uniques = search._factorize(flat)
    return lens, codes, uniques


class Corpus(object):
    """The fan works as ids: `names`, `work_off` (uint64, n_works + 1), `raw` (per token the
    number of its text as written, into `texts`) and `fold_of` (per text the dense id of its
    folded form: what the library compares).  Every distinct text is held once."""

    def __init__(self, names, keep_case=False, workers=None):
        from . import search
        self.names = list(names)
        self.keep_case = bool(keep_case)
        self.texts, self._raw_id = [], {}
        self._fold_id = {}
        fold_of, lens, parts = [], [], []
        chunks = [self.names[i:i + CHUNK] for i in range(0, len(self.names), CHUNK)]
        workers = search.default_workers() if workers is None else workers
        pool = None
        if workers > 1 and len(chunks) > 1:
            import multiprocessing
            pool = multiprocessing.get_context("fork").Pool(min(workers, len(chunks)))
        try:
            for ln, codes, uniques in (pool.imap(_read_chunk, chunks) if pool
                                       else map(_read_chunk, chunks)):
                local = np.zeros(len(uniques), dtype=np.uint32)
                for j, t in enumerate(uniques):
                    r = self._raw_id.get(t)
                    if r is None:
                        r = self._raw_id[t] = len(self.texts)
                        self.texts.append(t)
                        fold_of.append(self._fold_id.setdefault(self.fold(t), len(self._fold_id)))
                    local[j] = r
                lens.append(ln)
                parts.append(local[codes] if len(codes) else np.zeros(0, np.uint32))
        finally:
            if pool is not None:
                pool.close()
                pool.join()
        self.raw = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        self.fold_of = np.asarray(fold_of, dtype=np.uint32)
        self.work_off = np.zeros(len(self.names) + 1, dtype=np.uint64)
        if lens:
            self.work_off[1:] = np.cumsum(np.concatenate(lens))
        self.n_ids = len(self._fold_id)

    def fold(self, text):
        return text if self.keep_case else text.lower()

    def tok(self):
        """The folded id of every token."""
        return self.fold_of[self.raw] if len(self.raw) else np.zeros(0, np.uint32)

    def script_ids(self, words):
        """The ids of a script's words; abi.FS_FANON_NO_ID for a word no fan token equals."""
        return np.asarray([self._fold_id.get(self.fold(w), abi.FS_FANON_NO_ID) for w in words],
                          dtype=np.uint32)

    def text(self, work, start, n):
        """Tokens start .. start + n of a work as written, joined by spaces."""
        b = int(self.work_off[work]) + int(start)
        return ' '.join(self.texts[r] for r in self.raw[b:b + int(n)].tolist())


def read_scripts(corpus, scripts):
    """(canon ids, canon_off) of the script markups: the LOWERCASE column of
    load_markup_script, folded as the fan tokens are.  Scripts do not join."""
    from . import search
    parts = [corpus.script_ids([r[0] for r in search.load_markup_script(s)[1:]]) for s in scripts]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint32)), off


def rank_phrases(phrases):
    """The phrases' indices by works descending, then most descending, then tokens descending,
    then first appearance (their order as the library gives them): one stable sort."""
    j = np.arange(len(phrases))
    return np.lexsort((j, -phrases['n_tokens'].astype(np.int64), -phrases['most'].astype(np.int64),
                       -phrases['n_works'].astype(np.int64)))


def rank_grams(grams):
    """The grams' indices by works descending, then occurrences descending, then first
    appearance."""
    j = np.arange(len(grams))
    return np.lexsort((j, -grams['occurrences'].astype(np.int64),
                       -grams['works'].astype(np.int64)))


def tables(corpus, canon, canon_off, length=8, min_works=2, max_share=100, top=1000, device=0):
    """The rows of the four CSVs, without headers: phrases, passages, grams, works."""
    from . import engine
    works, grams, passages, phrases, _ = engine.fanon(
        corpus.tok(), corpus.work_off, corpus.n_ids, canon, canon_off, length, min_works,
        max_share, device)
    names = corpus.names
    order = rank_phrases(phrases)
    if top:
        order = order[:top]
    rank_of = np.zeros(len(phrases), dtype=np.int64)          # 0: cut by --top
    rank_of[order] = np.arange(1, len(order) + 1)
    t_phrases = []
    for r, j in enumerate(order.tolist()):
        f = phrases[j]
        t_phrases.append([r + 1, int(f['n_tokens']), int(f['n_works']), int(f['n_passages']),
                          int(f['least']), int(f['most']), names[int(f['work'])],
                          int(f['start']), corpus.text(f['work'], f['start'], f['n_tokens'])])
    t_passages = []
    for p in passages:
        rank = int(rank_of[int(p['phrase'])])
        t_passages.append([names[int(p['work'])], int(p['start']),
                           int(p['start']) + int(p['n_tokens']) - 1, int(p['n_tokens']),
                           rank if rank else '', int(p['least']), int(p['most']),
                           corpus.text(p['work'], p['start'], p['n_tokens'])])
    g_order = rank_grams(grams)
    if top:
        g_order = g_order[:top]
    t_grams = []
    for r, j in enumerate(g_order.tolist()):
        g = grams[j]
        t_grams.append([r + 1, int(g['works']), int(g['occurrences']), names[int(g['work'])],
                        int(g['start']), corpus.text(g['work'], g['start'], length)])
    t_works = []
    for w, r in enumerate(works):
        t_works.append([names[w], int(r['n_tokens']), int(r['n_positions']),
                        int(r['shared_positions']), int(r['canon_positions']),
                        int(r['common_positions']), int(r['n_passages']),
                        int(r['shared_tokens']), int(r['canon_tokens']),
                        int(r['longest_start']) if int(r['n_passages']) else '',
                        int(r['longest_tokens']),
                        corpus.text(w, r['longest_start'], r['longest_tokens'])])
    return t_phrases, t_passages, t_grams, t_works


def output_names(directory, prefix=None):
    """The four files: `prefix` (default: the directory's base name) in front of each suffix."""
    if prefix is None:
        prefix = os.path.basename(os.path.normpath(directory))
    return tuple(prefix + s for s in ('-fanon.csv', '-fanon-passages.csv', '-fanon-grams.csv',
                                      '-fanon-works.csv'))


def process(args):
    """`ao3.py fanon fan_works [script ...] [-o PREFIX] [--length K] [--min-works W]
    [--max-share P] [--keep-case] [--top N] [-n N] [-s S] [--listing sorted|os] [--device D]`."""
    from . import search
    names = search.list_fan_works(args.fan_works, args.skip_works, args.num_works, args.listing)
    corpus = Corpus(names, args.keep_case)          # (the pool forks before the GPU is touched)
    canon, canon_off = read_scripts(corpus, args.scripts)
    outs = output_names(args.fan_works, args.output)
    write_tables(outs, (PHRASE_FIELDS, PASSAGE_FIELDS, GRAM_FIELDS, WORK_FIELDS),
                 tables(corpus, canon, canon_off, args.length, args.min_works, args.max_share,
                        args.top, args.device))
    return outs
