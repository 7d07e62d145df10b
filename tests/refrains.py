"""Scripts that repeat a line with a word changed (refrains), for the one-slot maps of the LSH
pipeline: plain numpy, no GPU.  test_refrains_host.py checks the cases here against the oracle,
test_gpu_refrains.py runs them on the device.

Two script n-grams that differ in one slot have the same one-slot-wildcard key for that slot
(fs_hash.h) and land in the same bucket of four of `wmap` (fs_lsh_build) and `emap` (build_emap):
the one place where those maps have data-dependent branches.  A script here is random filler
(synth.script_tokens) with refrains spliced in between stretches of filler; a refrain is a base
line of n tokens with the words at chosen slots replaced by chosen variants, each form occurring
a chosen number of times.  The fan works (synth.fanwork_tokens) hold the line with a word the
script never has at that slot (near: within the threshold of some form; far: of none), a form
verbatim, and forms with two slots changed, which must give no record.

The module restates, in integers, fs_premix / fs_rotl / fs_rot_of / fs_wild_key / fs_wmap_slot
and how the two vector-id maps are sized and filled.  How many entries a bucket ends up with
does not depend on the order of insertion under linear probing, so the restatement says which
buckets are full and how long a chain of full buckets is without knowing gram ids; it is used
to place a refrain (`chain_case`) and to assert the layout a case names (`layout_of`).  It also
restates which script n-grams the reference's LSH finds for a window (`plan`): the n-grams one
slot away, their cosine distance in float64, and the tables whose key they share with the window.
"""

import functools

import numpy as np

from fandom_search_amd import abi, synth
from fandom_search_amd.vocab import pack_strings

ROWS = 3000                     # the first rows of the tables, as the other LSH tests take them
THR = 0.1
H, B = 15, 14
_M = 0xFFFFFFFF


# ---- fs_hash.h, restated (Python ints, or numpy uint64 arrays holding 32-bit values) ----------

def premix(t):
    return ((t & 0xFFFFFF) * 0x9E3779) & _M


def rotl(x, r):
    r = r & 31
    return ((x << r) | (x >> ((32 - r) & 31))) & _M


def rot_of(j):
    return (7 * j) & 31


def wild_key(fold_all, term_j, j):
    h = ((fold_all ^ term_j) + 0x9E3779B9 * (j + 1)) & _M
    h = h ^ (h >> 15)
    h = (h * 0x85EBCA6B) & _M
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M
    return h ^ (h >> 16)


def wmap_slot(h, log2_slots):
    return ((h * 0x9E3779B1) & _M) >> (32 - log2_slots)


def wild_group(k, n):
    return 3 * k // n


def window_keys(ids):
    """The n one-slot-wildcard keys of one window."""
    n = len(ids)
    term = [rotl(premix(int(t)), rot_of(n - 1 - k)) for k, t in enumerate(ids)]
    fold = 0
    for t in term:
        fold ^= t
    return [wild_key(fold, term[k], k) for k in range(n)]


def all_window_keys(ids, n):
    """[W][n] keys of every window of the id sequence (uint64 holding 32-bit values)."""
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(ids, dtype=np.uint64), n)
    rot = np.array([rot_of(n - 1 - k) for k in range(n)], dtype=np.uint64)
    term = rotl(premix(win), rot[None, :])
    fold = np.bitwise_xor.reduce(term, axis=1)
    j = np.arange(n, dtype=np.uint64)[None, :]
    return wild_key(fold[:, None], term, j)


# ---- the maps' layout, restated --------------------------------------------------------------

def distinct_grams(script, n):
    """First window of every distinct script n-gram (by vector ids), and every window's n-gram
    as an index into them."""
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(script, dtype=np.uint32), n)
    _, first, inverse = np.unique(win, axis=0, return_index=True, return_inverse=True)
    return first, np.asarray(inverse).reshape(-1)


class OneSlotMap(object):
    """Buckets of four, a full bucket spilling into the next: entries per bucket (`fill`), and
    the bucket every entry went to, in the order the keys are given (`bucket`)."""

    def __init__(self, keys, log2):
        self.log2 = log2
        self.mask = (1 << log2) - 1
        self.fill = np.zeros(1 << log2, dtype=np.int64)
        self.bucket = []
        for h in keys:
            b = self.home(int(h))
            while self.fill[b] == 4:
                b = (b + 1) & self.mask
            self.fill[b] += 1
            self.bucket.append(b)
        self.entry = {}                                # (first window of the n-gram, slot) -> entry number

    def depth(self, window, slot, h):
        """Buckets between the key's home and where the n-gram's entry for `slot` lies."""
        return (self.bucket[self.entry[(int(window), int(slot))]] - self.home(h)) & self.mask

    def home(self, h):
        return int(wmap_slot(int(h), self.log2))

    def chain(self, h):
        """Full buckets in a row from the key's home bucket on."""
        b, m = self.home(h), 0
        while self.fill[(b + m) & self.mask] == 4 and m <= self.mask:
            m += 1
        return m


def map_sizes(n_grams, n):
    """log2 of the buckets of wmap (2^lm >= entries) and of emap (2^lm >= 2 G n)."""
    lw = 8
    while lw < 26 and (1 << lw) < n_grams * n:
        lw += 1
    le = 8
    while le < 26 and (1 << le) < 2 * n_grams * n:
        le += 1
    return lw, le


def layout_of(script, n):
    """(wmap, emap) of the script by vector ids: one entry per distinct n-gram and slot, put in
    in the builders' order -- wmap by the n-grams in lexicographic order of their ids
    (fs_lsh_build), emap by gram id, which is the memcmp order of the ids' bytes
    (build_gram_index); an n-gram's slots in ascending order."""
    first, _ = distinct_grams(script, n)                # (np.unique: lexicographic order of the rows)
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(script, dtype=np.uint32), n)
    by_bytes = sorted(first, key=lambda w: win[w].astype("<u4").tobytes())
    allk = all_window_keys(script, n)
    lw, le = map_sizes(len(first), n)
    maps = []
    for order, log2 in ((first, lw), (by_bytes, le)):
        m = OneSlotMap(allk[np.asarray(order, dtype=np.int64)].reshape(-1), log2)
        m.entry = {(int(w), k): i * n + k for i, w in enumerate(order) for k in range(n)}
        maps.append(m)
    return maps[0], maps[1]


# ---- tables ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def synthetic():
    """The synthetic table's first ROWS rows, their words and the cosines of all pairs."""
    emb = np.ascontiguousarray(synth.embedding()[:ROWS])
    words = synth.vocab_words()[:ROWS]
    cos = emb.astype(np.float64) @ emb.astype(np.float64).T
    np.fill_diagonal(cos, -2.0)
    return emb, words, cos


@functools.lru_cache(maxsize=None)
def clustered():
    """synth.clustered_table's first ROWS rows, their words, and the cluster of every row."""
    emb, perm = synth.clustered_table()
    cluster = np.empty(len(emb), dtype=np.int64)
    cluster[perm] = np.arange(len(emb)) // 8
    return np.ascontiguousarray(emb[:ROWS]), synth.vocab_words()[:ROWS], cluster[:ROWS]


@functools.lru_cache(maxsize=None)
def normals_of(n):
    return synth.lsh_normals(n, H, B)


def lsh_bits(emb, n, ids):
    """The H x B key bits of a window (float64 projections of the concatenated vectors)."""
    v = emb[np.asarray(ids, dtype=np.int64)].astype(np.float64).reshape(-1)
    return (normals_of(n).reshape(H * B, -1) @ v > 0.0).reshape(H, B)


def distance(emb, a, b):
    """Cosine distance of two windows, float64."""
    u = emb[np.asarray(a, dtype=np.int64)].astype(np.float64).reshape(-1)
    v = emb[np.asarray(b, dtype=np.int64)].astype(np.float64).reshape(-1)
    return 1.0 - float(u @ v) / float(np.sqrt(u @ u) * np.sqrt(v @ v))


def line_cosine(n):
    """The cosine two unit vectors need for the one slot in which two windows differ."""
    return 1.0 - n * THR


# ---- assembling a case -------------------------------------------------------------------------

def refrain(base, forms, fans):
    """base: n ids; forms: [(slot -> id, occurrences)] of the script; fans: [(slot -> id, kind)],
    kind one of "near", "far", "verbatim", "two"."""
    return dict(base=[int(t) for t in base], forms=list(forms), fans=list(fans))


def _with(base, subst):
    line = list(base)
    for k, t in subst.items():
        line[k] = int(t)
    return line


FAN_WORK = 300
FAN_STEP = 40                   # a planted window every FAN_STEP tokens of a fan work, from token 20


def assemble(table, n, refrains, nearest_n=10, unique=1, filler_len=1200, seed=1):
    """The case: script (filler with the refrains' lines between stretches of it, in a shuffled
    order), script words (some spelt differently from the table), fan works, and where every
    planted fan window sits."""
    emb, words = table[0], table[1]
    rng = np.random.default_rng(seed)
    lines = []
    for r, ref in enumerate(refrains):
        for subst, occ in ref["forms"]:
            lines += [_with(ref["base"], subst)] * occ
    order = rng.permutation(len(lines))
    filler = synth.script_tokens(filler_len, ROWS, seed=synth.SCRIPT_SEED + seed)
    assert 600 <= filler_len <= 2000 and filler_len >= (len(lines) + 1) * (n + 4)
    cuts = np.linspace(0, filler_len, len(lines) + 2).astype(np.int64)
    parts = []
    for j, li in enumerate(order):
        parts += [filler[cuts[j]:cuts[j + 1]], np.asarray(lines[li], dtype=np.uint32)]
    parts.append(filler[cuts[len(lines)]:])
    script = np.concatenate(parts).astype(np.uint32)
    # (the Levenshtein distance of a match with the script window's ids is not a constant)
    swords = [words[int(t)].upper() if i % 7 == 0 else words[int(t)] for i, t in enumerate(script)]
    fans = [(r, _with(ref["base"], subst), kind) for r, ref in enumerate(refrains) for subst, kind in ref["fans"]]
    per = (FAN_WORK - 20 - n) // FAN_STEP
    n_works = max(3, -(-len(fans) // per))
    tok = np.concatenate([synth.fanwork_tokens(w, FAN_WORK, script, ROWS) for w in range(n_works)]).astype(np.uint32)
    planted = []
    # two words the script does not have, on both sides of a window with two slots changed: a
    # window that covers only some of its tokens then differs from every script window in two
    # slots as well, whatever the fan work's own words are
    absent = np.setdiff1d(np.arange(ROWS, dtype=np.uint32), script)[:2]
    for j, (r, line, kind) in enumerate(fans):
        at = (j // per) * FAN_WORK + 20 + (j % per) * FAN_STEP
        tok[at:at + n] = line
        if kind == "two":
            tok[at - 2:at] = absent
            tok[at + n:at + n + 2] = absent
        planted.append(dict(refrain=r, pos=at, work=j // per, fan_ix=at % FAN_WORK, ids=line, kind=kind))
    off = np.arange(n_works + 1, dtype=np.uint64) * np.uint64(FAN_WORK)
    chars, coff = pack_strings(words)
    return dict(n=n, emb=emb, words=words, script=script, swords=swords, tok=tok, off=off, chars=chars, coff=coff,
                normals=normals_of(n), nearest_n=nearest_n, unique=unique, refrains=refrains, planted=planted,
                key_ids=table[2] if len(table) > 2 and table[2].dtype.kind == "i" else None)


def config_of(case):
    return abi.make_config(window_size=case["n"], number_of_hashes=H, hash_dimensions=B, distance_threshold=THR,
                           nearest_n=case["nearest_n"], unique_filter=case["unique"])


def oracle_rows(case, threads=8):
    from oracle import c_oracle
    sch, so = pack_strings(case["swords"])
    oi = c_oracle.OracleIndex(config_of(case), case["script"], sch, so, case["emb"], case["normals"], threads=threads)
    return oi.search(case["tok"], case["off"], case["chars"], case["coff"])


def rows_at(rows, fan):
    """The records on the tokens of a planted window."""
    n = len(fan["ids"])
    sel = (rows["work"] == fan["work"]) & (rows["fan_ix"] >= fan["fan_ix"]) & (rows["fan_ix"] < fan["fan_ix"] + n)
    return rows[sel]


# ---- what the maps and the LSH hold for a planted window ---------------------------------------

def plan(case, every=False):
    """Per planted window (every: per window of the fan works that equals a script n-gram in all
    slots but one at most): the distinct script n-grams that equal it in all slots but one (by
    the ids the maps are keyed by), in the order k_lsh_enum meets them (by slot), each with its
    slot, occurrences, distance, and the tables whose key it shares with the window."""
    n, script, emb = case["n"], case["script"], case["emb"]
    key_ids = case["key_ids"]
    sk = script if key_ids is None else key_ids[script]
    win = np.lib.stride_tricks.sliding_window_view(script, n)
    kwin = np.lib.stride_tricks.sliding_window_view(sk, n)
    first, gram = distinct_grams(script, n)
    occ = np.bincount(gram, minlength=len(first))
    out = []
    fans = case["planted"]
    if every:
        kind = {p["pos"]: p["kind"] for p in case["planted"]}
        tk = case["tok"] if key_ids is None else key_ids[case["tok"]]
        fans = []
        for w in range(len(case["off"]) - 1):
            lo, hi = int(case["off"][w]), int(case["off"][w + 1])
            if hi - lo < n:
                continue
            fw = np.lib.stride_tricks.sliding_window_view(tk[lo:hi], n)
            same = np.zeros((len(first), len(fw)), dtype=np.int16)
            for k in range(n):
                same += kwin[first][:, k][:, None] == fw[:, k][None, :]
            for j in np.nonzero((same >= n - 1).any(axis=0))[0]:
                at = lo + int(j)
                fans.append(dict(refrain=-1, pos=at, work=w, fan_ix=int(j), kind=kind.get(at, "other"),
                                 ids=[int(t) for t in case["tok"][at:at + n]]))
    for fan in fans:
        f = np.asarray(fan["ids"], dtype=np.uint32)
        fk = f if key_ids is None else key_ids[f]
        same = (kwin[first] == fk[None, :]).sum(axis=1)
        fbits = lsh_bits(emb, n, f)
        grams = []
        for g in np.nonzero(same >= n - 1)[0]:
            w = int(first[g])
            exact = bool((win[w] == f).all())
            slot = -1 if same[g] == n else int(np.nonzero(kwin[w] != fk)[0][0])
            tables = [int(h) for h in np.nonzero((lsh_bits(emb, n, win[w]) == fbits).all(axis=1))[0]]
            grams.append(dict(window=w, slot=slot, exact=exact, occ=int(occ[g]), dist=distance(emb, win[w], f),
                              tables=tables))
        grams.sort(key=lambda e: (e["slot"], e["window"]))
        listed = [e for e in grams if not e["exact"] and e["dist"] < THR and e["tables"]]
        out.append(dict(fan=fan, grams=grams, one_slot=[e for e in grams if not e["exact"]], listed=listed,
                        is_gram=any(e["exact"] for e in grams)))
    return out


def wanted_entries(entry, unique, nearest_n, kept=False):
    """Entries of the neighbour list the listed n-grams of a planned window ask for (the list
    keeps nearest_n): an n-gram once per table that shares its key, every occurrence each time;
    with the UniqueFilter in the first such table only.  kept: as the index sees it, which keeps
    the first nearest_n occurrences of an n-gram and no count beyond them (build_gram_index)."""
    return sum((1 if unique else len(e["tables"])) * (min(e["occ"], nearest_n) if kept else e["occ"])
               for e in entry["listed"])


# ---- the cases ---------------------------------------------------------------------------------

# the counters of fs_index_lsh_counts (ScriptIndex.LSH_COUNT_NAMES) a case is there for: by the
# number of forms in one slot, by the length of the chain, by the number of respellings
FORMS = {1: ("wmap_ended_1", "wmap_pending_distance", "enum_listed_1"),
         2: ("wmap_ended_2", "wmap_pending_distance", "enum_listed_2"),
         3: ("wmap_pending_many", "enum_listed_3"),
         4: ("wmap_pending_full_bucket", "enum_listed_4", "enum_chain_once"),
         5: ("wmap_pending_full_bucket", "enum_giveup_fifth", "enum_chain_once")}
CHAINS = {1: "enum_chain_once", 2: "enum_chain_twice", 3: "enum_giveup_chain"}
COMPONENTS = {2: ("enum_listed_2",), 4: ("enum_listed_4", "enum_chain_once"), 5: ("enum_giveup_fifth", "enum_chain_once")}

def slots_of(n):
    """Slot 0, the middle, n - 1, and the slots on both sides of the borders of fs_wild_group."""
    s = {0, n // 2, n - 1}
    for k in range(1, n):
        if wild_group(k, n) != wild_group(k - 1, n):
            s |= {k - 1, k}
    return sorted(s)


def _far_word(cos, rng, avoid, n):
    """A row below the line against every word of `avoid`: one of the five lowest."""
    worst = cos[:, avoid].max(axis=1)
    worst[avoid] = 2.0
    r = int(np.argsort(worst)[int(rng.integers(0, 5))])
    assert worst[r] < line_cosine(n) - 0.01, (worst[r], n)
    return r


def _base_line(rng, n, avoid):
    while True:
        base = [int(t) for t in rng.integers(0, ROWS, size=n)]
        if len(set(base)) == n and not set(base) & set(avoid):
            return base


def forms_case(n, v, unique=1, seed=1):
    """V forms of a line in one slot, each once; a refrain per slot of slots_of(n).  The forms'
    words at slot k are the rows nearest to one word y, which the near fan window carries there
    (above the line for all of them where the table has such a y: the list then holds V
    n-grams); the far window carries a row below the line against every form."""
    table = synthetic()
    cos = table[2]
    rng = np.random.default_rng(1000 * n + 10 * v + seed)
    # the words with the most rows well above the line: by their V-th largest cosine
    vth = -np.sort(-cos, axis=1)[:, min(v, 4) - 1]
    ys = [int(y) for y in np.argsort(-vth)[:len(slots_of(n))]]
    refrains = []
    for k, y in zip(slots_of(n), ys):
        fam = [int(x) for x in np.argsort(-cos[y])[:v]]
        base = _base_line(rng, n, fam + [y])
        far = _far_word(cos, rng, fam + [y], n)
        k2 = (k + 1 + int(rng.integers(0, n - 2))) % n
        k3 = (k2 + 1) % n if (k2 + 1) % n != k else (k2 + 2) % n
        two = _far_word(cos, rng, [base[k2]], n)
        two3 = _far_word(cos, rng, [base[k3]], n)
        refrains.append(refrain(base, [({k: x}, 1) for x in fam],
                                [({k: y}, "near"), ({k: far}, "far"), ({k: fam[0]}, "verbatim"),
                                 ({k: y, k2: two}, "two"), ({k: fam[-1], k2: two, k3: two3}, "two")]))
    return assemble(table, n, refrains, unique=unique, seed=seed)


ORDERS = {"ascending": (0, 1, 2, 3), "descending": (3, 2, 1, 0), "interleaved_a": (1, 3, 0, 2),
          "interleaved_b": (2, 0, 3, 1)}


def slots_case(n, order, unique=1, seed=1, nearest_n=10):
    """Forms at different slots: the fan window F is one slot from each of two, three and four
    script n-grams, through as many different keys (the script holds F with slot s_m changed
    to w_m, never F).  The substitutes' cosines are graded, so the distances arrive -- by slot
    -- in the rank order `order` names; every line is redrawn until the reference's LSH holds
    all its n-grams in a table shared with F.  At nearest_n = 1, 2, 3 the list holds fewer places
    than n-grams (each occurs once): the order decides which of them are kept."""
    table = synthetic()
    emb, _, cos = table
    rng = np.random.default_rng(2000 * n + seed)
    best = cos.argmax(axis=1)
    top = cos.max(axis=1)
    # pairs (y, nearest row) well above the line, each word once
    pairs, used = [], set()
    for y in np.argsort(-top):
        y, x = int(y), int(best[y])
        if y in used or x in used or top[y] < line_cosine(n) + 0.02:
            continue
        pairs.append((y, x, float(top[y])))
        used |= {y, x}
        if len(pairs) == 40:
            break
    refrains = []
    at = 0
    for count in (4, 4, 4, 3, 2):
        rank = [r for r in ORDERS[order] if r < count]
        slots = slots_of(n)[::2][:count] if count < 4 else [0, n // 2 - 1, n // 2 + 1, n - 1]
        for _ in range(200):
            mine = sorted(pairs[at::10][:count], key=lambda p: -p[2])       # rank 0: the nearest
            at = (at + 1) % 10
            line = _base_line(rng, n, [t for p in mine for t in p[:2]])
            for s, r in zip(slots, rank):
                line[s] = mine[r][0]
            forms = [({s: mine[r][1]}, 1) for s, r in zip(slots, rank)]
            fbits = lsh_bits(emb, n, line)
            if all((lsh_bits(emb, n, _with(line, sub)) == fbits).all(axis=1).any() for sub, _ in forms):
                break
        else:
            raise AssertionError("no line whose n-grams share a table with the window")
        k2, k3 = [k for k in range(n) if k not in slots][:2]
        two = {k2: _far_word(cos, rng, [line[k2]], n), k3: _far_word(cos, rng, [line[k3]], n)}
        refrains.append(refrain(line, forms, [({}, "near"), ({**forms[0][0], **two}, "two")]))
    return assemble(table, n, refrains, nearest_n=nearest_n, unique=unique, seed=seed)


OCCURRENCES = (1, 3, 10, 12)


def occurrences_case(n, nearest_n, unique, seed=1):
    """A form occurring 1, 3, 10 and 12 times next to a second form in the same slot occurring
    twice; lines redrawn until the LSH holds both in a table shared with the near fan window.
    The nearer form's entries come first and the other gets the places that are left: the
    nearer one is the form of 1, 3 and 12 occurrences, and the one of two next to the form of
    10 -- so N = 3 ends a list between two n-grams and inside one, N = 10 inside one (12) and
    with the second n-gram taking the eight places left (2 + 10)."""
    table = synthetic()
    emb, _, cos = table
    rng = np.random.default_rng(3000 * n + seed)
    second = -np.sort(-cos, axis=1)[:, 1]
    ys = [int(y) for y in np.argsort(-second)[:len(OCCURRENCES)]]
    refrains = []
    for occ, y, k in zip(OCCURRENCES, ys, slots_of(n)[1:]):
        fam = [int(x) for x in np.argsort(-cos[y])[:2]]
        for _ in range(200):
            base = _base_line(rng, n, fam + [y])
            fbits = lsh_bits(emb, n, _with(base, {k: y}))
            if all((lsh_bits(emb, n, _with(base, {k: x})) == fbits).all(axis=1).any() for x in fam):
                break
        else:
            raise AssertionError("no line whose forms share a table with the window")
        if occ == 10:
            fam.reverse()                               # (fam[0] is the nearer one to y)
        refrains.append(refrain(base, [({k: fam[0]}, occ), ({k: fam[1]}, 2)],
                                [({k: y}, "near"), ({k: fam[0]}, "verbatim")]))
    return assemble(table, n, refrains, nearest_n=nearest_n, unique=unique, filler_len=2000, seed=seed)


def own_record_case(n, unique=1, seed=1):
    """The fan window is a script form verbatim, and the script holds another form within the
    threshold in a shared table: the record of k_lsh_gramtab with further matches."""
    table = synthetic()
    emb, _, cos = table
    rng = np.random.default_rng(4000 * n + seed)
    best = cos.argmax(axis=1)
    refrains = []
    for k, a in zip(slots_of(n), np.argsort(-cos.max(axis=1))[:len(slots_of(n))]):
        a, b = int(a), int(best[a])
        for _ in range(200):
            base = _base_line(rng, n, [a, b])
            if (lsh_bits(emb, n, _with(base, {k: a})) == lsh_bits(emb, n, _with(base, {k: b}))).all(axis=1).any():
                break
        else:
            raise AssertionError("no line whose forms share a table")
        refrains.append(refrain(base, [({k: a}, 1), ({k: b}, 2)], [({k: a}, "verbatim"), ({k: b}, "verbatim")]))
    return assemble(table, n, refrains, unique=unique, seed=seed)


def _stuffer(rng, n, log2, bucket, avoid):
    """Four forms of a line in one slot whose key's home bucket (of 2^log2) is `bucket`: a word
    of another slot is tried over the whole table at once, line after line."""
    k, kv = 1, 2
    for _ in range(400):
        base = _base_line(rng, n, avoid)
        if base[0] & 0xFF == 0xFF:                      # (the line they stand in front of has such a first id)
            continue
        term = [rotl(premix(t), rot_of(n - 1 - j)) for j, t in enumerate(base)]
        rest = 0
        for j in range(n):
            if j != k and j != kv:
                rest ^= term[j]
        cand = np.arange(ROWS, dtype=np.uint64)
        tv = rotl(premix(cand), rot_of(n - 1 - kv))
        # (fold_all ^ term_k: the fold of the other slots)
        keys = wild_key(np.uint64(rest) ^ tv, np.uint64(0), k)
        hit = np.nonzero(wmap_slot(keys, log2) == np.uint64(bucket))[0]
        hit = [int(t) for t in hit if int(t) not in base and int(t) not in avoid]
        if hit:
            base[kv] = hit[0]
            words = []
            while len(words) < 4:
                t = int(rng.integers(0, ROWS))
                if t not in base and t not in words and t not in avoid:
                    words.append(t)
            return refrain(base, [({k: t}, 1) for t in words], [])
    raise AssertionError("no line for bucket %d" % bucket)


def chain_case(n, length, unique=1, seed=1):
    """A line (one form, a near fan window) whose key's home bucket in emap starts a chain of
    `length` full buckets, with the line's own entry `length` buckets on: found at the first
    follow, at the second, or not (give-up by the chain).  Filler holds no such chains, so the
    buckets are filled by four-form refrains placed there through the restated map; emap takes
    its entries in by gram id, the memcmp order of the ids' bytes, so the line's first id has
    the low byte 0xFF and the refrains' have not: their entries are there first and the line's
    spills past them.  The restated map, which puts the entries in in that order, says where it
    lies (case["chain_depth"]).  wmap has half as many buckets of the same hash: the line's home
    bucket there is full as well."""
    table = synthetic()
    emb, _, cos = table
    rng = np.random.default_rng(5000 * n + 10 * length + seed)
    k = n // 2
    y = int(np.argsort(-cos.max(axis=1))[3])
    x = int(cos[y].argmax())
    for attempt in range(20):
        for _ in range(400):
            base = _base_line(rng, n, [x, y])
            base[0] = 0xFF + 0x100 * int(rng.integers(0, ROWS // 0x100))
            if len(set(base)) == n and base[0] not in (x, y) and \
                    (lsh_bits(emb, n, _with(base, {k: x})) == lsh_bits(emb, n, _with(base, {k: y}))).all(axis=1).any():
                break
        else:
            raise AssertionError("no line that shares a table with the window")
        target = refrain(base, [({k: x}, 1)], [({k: y}, "near"), ({k: x}, "verbatim")])
        # the maps' sizes follow from the number of distinct n-grams: a draft with any stuffers
        draft = [target] + [refrain(_base_line(rng, n, [x, y]), [({1: t}, 1) for t in range(4)], [])
                            for _ in range(length)]
        case = assemble(table, n, draft, unique=unique, seed=seed + attempt)
        _, le = map_sizes(len(distinct_grams(case["script"], n)[0]), n)
        h = window_keys(_with(base, {k: x}))[k]
        b = int(wmap_slot(h, le))
        refs = [target] + [_stuffer(rng, n, le, (b + m) & ((1 << le) - 1), [x, y] + base) for m in range(length)]
        case = assemble(table, n, refs, unique=unique, seed=seed + attempt)
        wmap, emap = layout_of(case["script"], n)
        line = np.asarray(_with(base, {k: x}), dtype=np.uint32)
        at = int(np.nonzero((np.lib.stride_tricks.sliding_window_view(case["script"], n) == line[None, :]).all(axis=1))[0][0])
        if emap.log2 == le and emap.chain(h) == length and wmap.chain(h) >= 1 and emap.depth(at, k, h) == length:
            case.update(chain_key=h, chain_slot=k, chain_window=at, chain_depth=emap.depth(at, k, h))
            return case
    raise AssertionError("no script with a chain of %d" % length)


# ---- the branches the planted windows take ------------------------------------------------------

# the counters a window takes only with a script n-gram one slot away: `predicted` is exact for
# them.  The others (a full bucket in the way, a chain) a window can also reach without one, where
# the filters in front let it through by a false positive: lower bounds.
EXACT = ("wmap_ended_1", "wmap_ended_2", "wmap_pending_distance", "wmap_pending_many",
         "enum_listed_1", "enum_listed_2", "enum_listed_3", "enum_listed_4", "enum_reordered", "enum_cut",
         "enum_giveup_fifth", "enum_giveup_tie")


def predicted(case, every=True):
    """The counters of fs_index_lsh_counts (ScriptIndex.LSH_COUNT_NAMES) for a case keyed by
    vector ids, from every window of the fan works that has a script n-gram one slot away or is
    one: the restated maps say which bucket is full, `plan` which n-grams are within the
    threshold and in a shared table.  Exact for the counters of EXACT, lower bounds for the rest.
    every = False: what the planted windows alone add."""
    assert case["key_ids"] is None
    n, unique, nearest_n = case["n"], case["unique"], case["nearest_n"]
    wmap, emap = layout_of(case["script"], n)
    c = {}

    def add(name):
        c[name] = c.get(name, 0) + 1

    for e in plan(case, every=every):
        keys = window_keys(e["fan"]["ids"])
        if e["is_gram"]:
            if e["listed"]:
                add("record_with_neighbours")
            continue
        one = e["one_slot"]
        # sift_stage2: a full bucket, more than two n-grams, a distance -- asked in this order
        if any(wmap.fill[wmap.home(h)] == 4 for h in keys):
            add("wmap_pending_full_bucket")
        elif len(one) > 2:
            add("wmap_pending_many")
        elif any(g["dist"] < THR for g in one):
            add("wmap_pending_distance")
        else:
            add("wmap_ended_%d" % len(one))
            continue
        # k_lsh_enum
        chains = [emap.chain(h) for h in keys]
        gave_up = False
        if max(chains) >= 3:
            add("enum_giveup_chain")
            gave_up = True
        elif max(chains) == 2:
            add("enum_chain_twice")
        elif max(chains) == 1:
            add("enum_chain_once")
        if len(one) > 4:
            add("enum_giveup_fifth")
            gave_up = True
        dists = [g["dist"] for g in e["listed"]]
        if len(set(dists)) < len(dists):
            add("enum_giveup_tie")
            gave_up = True
        if gave_up or not dists:
            continue
        add("enum_listed_%d" % len(dists))
        # arrival: by slot, then along the key's chain, then by the order the entries went in; the
        # kernel's network of five comparators over them, an n-gram that is not listed behind any
        # that is -- the counter says that one of them exchanged two listed n-grams
        arrive = sorted(one, key=lambda g: (g["slot"], emap.depth(g["window"], g["slot"], keys[g["slot"]]),
                                            emap.entry[(g["window"], g["slot"])]))
        gd = [g["dist"] for g in arrive] + [0.0] * (4 - len(arrive))
        gt = [g in e["listed"] for g in arrive] + [False] * (4 - len(arrive))
        exchanged = False
        for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
            if gt[b] and (not gt[a] or gd[b] < gd[a]):
                exchanged = exchanged or gt[a]
                gd[a], gd[b], gt[a], gt[b] = gd[b], gd[a], gt[b], gt[a]
        if exchanged:
            add("enum_reordered")
        if wanted_entries(e, unique, nearest_n, kept=True) > nearest_n:
            add("enum_cut")
    return c


# ---- a tie, component ids, the share rule's room ---------------------------------------------------

TIE_ROWS = (ROWS - 3, ROWS - 2, ROWS - 1)          # Y, X1, X2 of tie_table


@functools.lru_cache(maxsize=None)
def tie_table():
    """A copy of the synthetic table with three unit rows planted: Y = u, X1 = 0.5 u + s v and
    X2 = 0.5 u - s v, s = sqrt(0.75), u and v on disjoint coordinates.  Every other row is zero
    there (and unit again), so u and v are orthogonal to the rest of the table: c_max = 0.5
    comes from the planted rows, and at n = 8 a neighbour still differs in one slot at most.
    g(X1, Y) and g(X2, Y) add the same products in the same order (the others are +0 and -0):
    the two distances are bit-equal."""
    emb, words, _ = synthetic()
    emb = emb.copy()
    su, sv = [0, 1], [2, 3]
    emb[:, su + sv] = 0.0
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    u = np.zeros(emb.shape[1], dtype=np.float32)
    v = np.zeros(emb.shape[1], dtype=np.float32)
    u[su] = (0.6, 0.8)
    v[sv] = (0.8, 0.6)
    sv32 = (np.sqrt(0.75) * v.astype(np.float64)).astype(np.float32)
    y, x1, x2 = TIE_ROWS
    emb[y] = u
    emb[x1] = np.float32(0.5) * u + sv32
    emb[x2] = np.float32(0.5) * u - sv32
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    cos = emb.astype(np.float64) @ emb.astype(np.float64).T
    np.fill_diagonal(cos, -2.0)
    return emb, words, cos


def canonical_distance(emb, s, f):
    """The reference's distance of script window s and fan window f as the oracle adds it up:
    float64, one addition after the other."""
    def dot(a, b):
        return float(np.cumsum(emb[a].astype(np.float64) * emb[b].astype(np.float64))[-1])
    ss = ff = sf = 0.0
    for a, b in zip(s, f):
        ss = ss + dot(a, a)
        ff = ff + dot(b, b)
        sf = sf + dot(a, b)
    return 1.0 - sf / (np.sqrt(ss) * np.sqrt(ff))


def tie_case(unique=1, seed=1):
    """n = 8: the script holds a line with X1 and with X2 at one slot, the fan window has Y
    there -- two listed n-grams at bit-equal distance, a refrain per slot of slots_of, each line
    redrawn until both forms share a table with the window."""
    n = 8
    table = tie_table()
    emb = table[0]
    y, x1, x2 = TIE_ROWS
    rng = np.random.default_rng(6000 + seed)
    refrains = []
    for k in slots_of(n):
        for _ in range(400):
            base = _base_line(rng, n, list(TIE_ROWS))
            fbits = lsh_bits(emb, n, _with(base, {k: y}))
            if all((lsh_bits(emb, n, _with(base, {k: x})) == fbits).all(axis=1).any() for x in (x1, x2)):
                break
        else:
            raise AssertionError("no line whose forms share a table with the window")
        refrains.append(refrain(base, [({k: x1}, 1), ({k: x2}, 1)], [({k: y}, "near"), ({k: x1}, "verbatim")]))
    return assemble(table, n, refrains, unique=unique, seed=seed)


def components_case(n, respellings, unique=1, seed=1):
    """The clustered table: the script repeats a line in `respellings` respellings -- other
    members of the same clusters at two slots, so the vector ids differ there and the component
    ids are equal in all n slots, and every form has the same n keys.  The fan window is yet
    another respelling."""
    table = clustered()
    emb, _, cluster = table
    rng = np.random.default_rng(7000 * n + 10 * respellings + seed)
    sizes = np.bincount(cluster)
    rich = [int(c) for c in np.nonzero(sizes >= respellings + 1)[0]]
    refrains = []
    for r, (ka, kb) in enumerate(((0, n - 1), (1, n // 2), (n // 2 - 1, n - 2))):
        for _ in range(200):
            ca, cb = (rich[int(i)] for i in rng.choice(len(rich), size=2, replace=False))
            ma, mb = np.nonzero(cluster == ca)[0], np.nonzero(cluster == cb)[0]
            base = _base_line(rng, n, [int(t) for t in ma] + [int(t) for t in mb])
            forms = [({ka: int(ma[i]), kb: int(mb[i])}, 1) for i in range(respellings)]
            fan = {ka: int(ma[respellings]), kb: int(mb[respellings])}
            fbits = lsh_bits(emb, n, _with(base, fan))
            if all((lsh_bits(emb, n, _with(base, sub)) == fbits).all(axis=1).any() for sub, _ in forms):
                break
        else:
            raise AssertionError("no line whose respellings share a table with the window")
        kc = [k for k in range(n) if k not in (ka, kb)]
        far = {kc[0]: int(rng.integers(0, ROWS)), kc[1]: int(rng.integers(0, ROWS))}
        refrains.append(refrain(base, forms, [(fan, "near"), (forms[0][0], "verbatim"), ({**fan, **far}, "two")]))
    return assemble(table, n, refrains, unique=unique, seed=seed)


SHARE_ROWS = 2000


def share_room_case(seed=1):
    """synth.realistic_table cut to SHARE_ROWS rows (norms as it makes them: on unit rows the
    component prefilter takes the index and k_share_scan does not run), n = 6.  One line 600 times
    in the script, back to back; a fan work quotes it copy after copy, every third copy with a
    word swapped for one of its inner group -- more than 256 windows in a row with several keys
    in the filter each, so the workgroup's lists of 512 keys have no room for all of them."""
    n = 6
    emb, group = synth.realistic_table(rows=SHARE_ROWS)
    words = synth.realistic_words(SHARE_ROWS)
    rng = np.random.default_rng(8000 + seed)
    norms = np.linalg.norm(emb, axis=1)
    ok = np.nonzero(norms > np.median(norms))[0]
    line = [int(t) for t in rng.choice(ok, size=n, replace=False)]
    filler = synth.script_tokens(600, SHARE_ROWS, seed=synth.SCRIPT_SEED + seed)
    script = np.concatenate([filler[:300], np.tile(np.asarray(line, dtype=np.uint32), 600), filler[300:]]).astype(np.uint32)
    swords = [words[int(t)].upper() if i % 7 == 0 else words[int(t)] for i, t in enumerate(script)]
    works = []
    for w in range(4):
        t = synth.fanwork_tokens(w, 420, script, SHARE_ROWS).astype(np.uint32)
        copies = (60, 12, 3, 0)[w]
        for j in range(copies):
            q = list(line)
            if j % 3 == 1:
                k = int(rng.integers(0, n))
                mates = np.nonzero((group[:, 2] == group[q[k], 2]) & (np.arange(SHARE_ROWS) != q[k]))[0]
                if len(mates):
                    q[k] = int(mates[int(rng.integers(0, len(mates)))])
            t[20 + n * j:20 + n * (j + 1)] = q
        works.append(t)
    off = np.arange(5, dtype=np.uint64) * np.uint64(420)
    chars, coff = pack_strings(words)
    return dict(n=n, emb=emb, words=words, script=script, swords=swords, tok=np.concatenate(works), off=off,
                chars=chars, coff=coff, normals=normals_of(n), nearest_n=10, unique=1, refrains=[], planted=[],
                key_ids=None, line=line)
