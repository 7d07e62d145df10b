"""Arbitrary Levenshtein operand pairs through the public search (test helper, no GPU).

Matching is by vector id and text is free on both sides, so a search can be made to compute
Levenshtein.distance(a, b) for any chosen pair of texts:

- the script is P*n distinct vector ids (a seeded permutation of the synthetic vocabulary):
  every script n-gram is unique and windows at different offsets share no id in any slot;
- fan work i holds exactly the n tokens script[i*n : i*n+n]: one window, equal to script
  window i*n and to no other;
- the script words' text and the fan tokens' strings are whatever the pair says.

The search must then return exactly n records for work i, with orig_ix = i*n + k and
lev = distance(" ".join(script words), "[" + ", ".join(fan words) + "]").

A `Pair` is (name, script word texts, fan word texts).  `cases(name)` gives the named case
lists that the host and the GPU tests share; `build` turns a list into the arrays of a search.
"""

import collections
import functools

import numpy as np

from fandom_search_amd import synth
from fandom_search_amd.vocab import pack_strings

Pair = collections.namedtuple("Pair", "name swords fwords")

LETTERS = "abcdefghijklmnopqrst"                 # "about 20 letters"
FOREIGN = "é世\U0001F600"              # e-acute, a CJK character, an astral code point
CONTENTS = ("identical", "disjoint", "repeat", "period2", "rand2", "rand20", "shifted", "foreign",
            "punct")
SPLITS = ("first", "last", "even", "random")
BIG_CONTENTS = ("disjoint", "rand2", "shifted")  # run on the whole product at n = 6
SUB_MAX = 129                                    # the sub-grid: both operands at or below this
WINDOW_SIZES = (1, 2, 4, 9, 12, 16)              # beside 6
FAN_WORD_LENGTHS = (0, 1, 14, 15, 16, 17, 254, 255, 256, 257, 300)
ALPHABET_SIZES = (124, 125, 126)


def la_grid(n):
    return sorted({v for v in (n - 1, n, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512) if v >= n - 1})


def lb_grid(n):
    return sorted({v for v in (2 * n, 2 * n + 1, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193,
                               511, 512) if v >= 2 * n})


def script_text(pair):
    return " ".join(pair.swords)


def fan_text(pair):
    return "[" + ", ".join(pair.fwords) + "]"


# ---- the reference ------------------------------------------------------------------------

def distance_plain(a, b):
    """Textbook unit-cost DP over code points, full table, plain Python integers."""
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def distance_rows(a, b):
    """The same DP a row at a time in numpy: cur[j] = min(t[j], cur[j-1] + 1) with
    t = min(prev[j] + 1, prev[j-1] + cost) is a running minimum of t[j] - j."""
    bb = np.array([ord(c) for c in b], dtype=np.int64)
    ramp = np.arange(len(b) + 1, dtype=np.int64)
    prev = ramp.copy()
    for i, ca in enumerate(a, 1):
        t = np.empty(len(b) + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (bb != ord(ca)))
        prev = np.minimum.accumulate(t - ramp) + ramp
    return int(prev[-1])


PLAIN_BELOW = 130        # operands under this many code points always take the plain DP


@functools.lru_cache(maxsize=None)
def distance(a, b):
    """Levenshtein.distance(a, b): unit costs over code points.  The numpy rows stand in where
    an operand has PLAIN_BELOW code points or more (test_levpairs_host.py holds them equal)."""
    if len(a) < PLAIN_BELOW and len(b) < PLAIN_BELOW:
        return distance_plain(a, b)
    return distance_rows(a, b)


def pair_distance(pair):
    return distance(script_text(pair), fan_text(pair))


# ---- shaping operands ---------------------------------------------------------------------

def split(text_len, n, how, rng=None):
    """Lengths of n words (zero allowed) that hold text_len characters in all."""
    if how == "first":
        return [text_len] + [0] * (n - 1)
    if how == "last":
        return [0] * (n - 1) + [text_len]
    if how == "even":
        return [text_len // n + (1 if k < text_len % n else 0) for k in range(n)]
    if how == "random":
        cuts = sorted(int(c) for c in rng.integers(0, text_len + 1, size=n - 1))
        edges = [0] + cuts + [text_len]
        return [edges[k + 1] - edges[k] for k in range(n)]
    raise ValueError(how)


def cut(text, lengths):
    out, at = [], 0
    for ln in lengths:
        out.append(text[at:at + ln])
        at += ln
    assert at == len(text)
    return out


def _draw(rng, alphabet, count):
    return "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=count))


def content(kind, rng, A, B):
    """Word characters of the two sides: A for the script, B for the fan work."""
    if kind == "identical":
        base = _draw(rng, LETTERS, max(A, B))
        return base[:A], base[:B]
    if kind == "disjoint":
        return _draw(rng, LETTERS[:10], A), _draw(rng, LETTERS[:10].upper(), B)
    if kind == "repeat":
        return "a" * A, "a" * B
    if kind == "period2":
        return ("ab" * A)[:A], ("ba" * B)[:B]
    if kind == "rand2":
        return _draw(rng, "ab", A), _draw(rng, "ab", B)
    if kind == "rand20":
        return _draw(rng, LETTERS, A), _draw(rng, LETTERS, B)
    if kind == "shifted":                       # first character dropped, one appended
        base = _draw(rng, LETTERS, A)
        return base, (base[1:] + _draw(rng, LETTERS, max(0, B - A + 1)))[:B]
    if kind == "foreign":                       # fan characters outside the script's alphabet
        base = _draw(rng, LETTERS, max(A, B))
        fan = list(base[:B])
        for j in range(0, B, 3):
            fan[j] = FOREIGN[(j // 3) % len(FOREIGN)]
        return base[:A], "".join(fan)
    if kind == "punct":                         # '[', ',' and ']' get classes of their own
        return _draw(rng, "ab[,]", A), _draw(rng, "ab[,]", B)
    raise ValueError(kind)


def make_pair(name, kind, n, la, lb, how_a, how_b, rng):
    A, B = la - (n - 1), lb - 2 * n
    assert A >= 0 and B >= 0, (n, la, lb)
    sa, sb = content(kind, rng, A, B)
    p = Pair(name, tuple(cut(sa, split(A, n, how_a, rng))), tuple(cut(sb, split(B, n, how_b, rng))))
    assert len(script_text(p)) == la and len(fan_text(p)) == lb
    return p


def grid(n, kinds, limit, seed, every_kind):
    """The product la_grid x lb_grid up to `limit`; every_kind: each cell once per kind, else
    the kinds take turns over the cells.  The split over the words changes from cell to cell."""
    rng = np.random.default_rng(seed)
    out = []
    cells = [(la, lb) for la in la_grid(n) if la <= limit for lb in lb_grid(n) if lb <= limit]
    for c, (la, lb) in enumerate(cells):
        for kind in (kinds if every_kind else (kinds[c % len(kinds)],)):
            how_a = SPLITS[len(out) % 4]
            how_b = SPLITS[(len(out) // 4) % 4]
            out.append(make_pair("%s n=%d la=%d lb=%d %s/%s" % (kind, n, la, lb, how_a, how_b),
                                 kind, n, la, lb, how_a, how_b, rng))
    return out


BASE16 = "abcdefghijklmnop"


def word_length_cases(n=6):
    """Fan words of the lengths where the string records change form, in the first, a middle
    and the last slot; at 15 and 16 the 15th and 16th characters decide the distance.
    Every fan text stays within 512 code points."""
    out = []
    for slot in (0, n // 2, n - 1):
        for L in FAN_WORD_LENGTHS:
            variants = [(BASE16 * 20)[:L]]
            if L == 15:
                variants += [BASE16[:14] + "Z", BASE16[:13] + "Zo"]
            if L == 16:
                variants += [BASE16[:15] + "Z", BASE16[:14] + "Zp", BASE16[:14] + "oZ"]
            if L >= 254:                                       # differences far behind the record
                variants += [(BASE16 * 20)[:L - 1] + "Z", "Z" + (BASE16 * 20)[1:L]]
            for v, fw in enumerate(variants):
                for sword in (BASE16, BASE16[:15]):
                    sw = ["xy"] * n
                    fws = ["xy"] * n
                    sw[slot] = sword
                    fws[slot] = fw
                    out.append(Pair("fan word of %d at slot %d, variant %d, script word of %d"
                                    % (L, slot, v, len(sword)), tuple(sw), tuple(fws)))
    return out


def long_fan_cases(n=6):
    """Fan texts past 512 code points against script windows within 64 (lane paths only)."""
    out = []
    rng = np.random.default_rng(77)
    for c, lens in enumerate(([300, 300, 0, 0, 0, 0], [0, 255, 256, 257, 0, 0], [254, 0, 0, 0, 0, 255],
                              [100, 100, 100, 100, 100, 100], [0, 0, 0, 0, 0, 600], [16, 15, 300, 17, 14, 256])):
        for kind in ("rand2", "shifted", "repeat"):
            A = (20, 40, 59)[c % 3]
            sa, sb = content(kind, rng, A, sum(lens))
            out.append(Pair("%s fan words %s" % (kind, lens), tuple(cut(sa, split(A, n, SPLITS[c % 4], rng))),
                            tuple(cut(sb, lens))))
    return out


def alphabet_cases(size, n=6, pairs=24):
    """A script whose text, the joining space included, has exactly `size` distinct code points."""
    rng = np.random.default_rng(size)
    alpha = "".join(chr(0x100 + i) for i in range(size - 1))    # (Latin Extended: none is a space)
    out = []
    every = alpha
    for i in range(pairs):
        A = (5 + 7 * i) % 60
        if every:                                               # the first pairs walk the alphabet
            sa, every = every[:59], every[59:]
            A = len(sa)
        else:
            sa = _draw(rng, alpha[-40:], A)                      # the highest classes
        kind = i % 3
        if kind == 0:
            sb = sa[1:] + alpha[-1]
        elif kind == 1:
            sb = "".join(FOREIGN[j % 3] if j % 4 == 0 else ch for j, ch in enumerate(sa)) + alpha[0]
        else:
            sb = _draw(rng, alpha[-3:] + alpha[:2], A + 9)
        out.append(Pair("alphabet %d pair %d" % (size, i), tuple(cut(sa, split(len(sa), n, SPLITS[i % 4], rng))),
                        tuple(cut(sb, split(len(sb), n, SPLITS[(i + 1) % 4], rng)))))
    return out


def alphabet_size(pairs):
    return len(set(" ") | set("".join(w for p in pairs for w in p.swords)))


def exact_distance_pair(n, want, slen=10):
    """Script window within 64 code points, fan text such that the distance is exactly `want`:
    the first fan word holds characters the script lacks, one more per unit of distance."""
    sw = tuple(["ab"] * (n - 1) + ["a" * slen])

    def pair(k):
        return Pair("distance %d" % want, sw, tuple(["B" * k] + [""] * (n - 1)))
    k = want
    d = pair_distance(pair(k))
    k += want - d
    p = pair(k)
    assert pair_distance(p) == want and len(script_text(p)) <= 64
    return p


def filler_pairs(n, count=8):
    return [Pair("filler %d" % i, tuple(["w%d" % i] * n), tuple(["W%d" % i] * n)) for i in range(count)]


@functools.lru_cache(maxsize=None)
def cases(name):
    """(window size, list of pairs) of a named case list."""
    if name.startswith("grid6_"):
        return 6, grid(6, (name[6:],), 512, 11, True)
    if name == "sub6_a":
        return 6, grid(6, ("identical", "repeat", "period2"), SUB_MAX, 12, True)
    if name == "sub6_b":
        return 6, grid(6, ("rand20", "foreign", "punct"), SUB_MAX, 13, True)
    if name.startswith("sub") and name[3:].isdigit():
        n = int(name[3:])
        return n, grid(n, CONTENTS, SUB_MAX, 20 + n, False)
    if name == "words6":
        return 6, word_length_cases(6)
    if name == "words6_long":
        return 6, long_fan_cases(6)
    if name.startswith("alpha"):
        return 6, alphabet_cases(int(name[5:]))
    if name in ("limit_d1023", "limit_d1024"):
        return 6, filler_pairs(6, 5) + [exact_distance_pair(6, int(name[7:]))] + filler_pairs(6, 3)
    if name in ("limit_la513_unquoted", "limit_la513_quoted"):
        p = make_pair("la=513", "rand2", 6, 513, 40, "even", "even", np.random.default_rng(5))
        if name.endswith("unquoted"):
            p = p._replace(name=UNQUOTED + " " + p.name)
        return 6, filler_pairs(6, 5) + [p] + filler_pairs(6, 3)
    if name == "limit_lb513":
        p = make_pair("lb=513", "rand2", 6, 20, 513, "even", "even", np.random.default_rng(6))
        return 6, filler_pairs(6, 5) + [p] + filler_pairs(6, 3)
    raise KeyError(name)


LIMIT_LISTS = ("limit_d1023", "limit_d1024", "limit_la513_unquoted", "limit_la513_quoted", "limit_lb513")


GRID_LISTS = tuple("grid6_" + k for k in BIG_CONTENTS) + ("sub6_a", "sub6_b")
WINDOW_LISTS = tuple("sub%d" % n for n in WINDOW_SIZES)
ALPHA_LISTS = tuple("alpha%d" % k for k in ALPHABET_SIZES)
WAVE_SAFE_LISTS = GRID_LISTS + WINDOW_LISTS + ("words6",) + ALPHA_LISTS    # both texts within 512
ALL_LISTS = WAVE_SAFE_LISTS + ("words6_long",)


# ---- from pairs to the arrays of a search ---------------------------------------------------

UNQUOTED = "unquoted"    # a pair whose name starts so gets an empty fan work: no record
SPACER_FROM = 250       # a pair with an operand longer than this is followed by a spacer pair


def with_spacers(pairs, n):
    """String id == vector id makes the library look at every script window with the strings of
    its own ids, the windows that straddle two pairs included: an empty pair on either side of
    every long one keeps those within the longer of the two texts."""
    out = []
    for p in pairs:
        long_one = max(len(script_text(p)), len(fan_text(p))) > SPACER_FROM
        if long_one and out and out[-1].name != "spacer":
            out.append(Pair("spacer", ("",) * n, ("",) * n))
        out.append(p)
        if long_one:
            out.append(Pair("spacer", ("",) * n, ("",) * n))
    return out


Built = collections.namedtuple(
    "Built", "n pairs script swords tok off chars coff tok_str work fan_ix orig_ix lev")


def build(pairs, n, layout, seed=1):
    """layout "own": string ids of their own (tok_str = arange into a table of P*n strings);
    "vec": string id == vector id, no tok_str (a table of one string per vocabulary id);
    "vec_explicit": the same table with tok_str == tok passed."""
    pairs = with_spacers(pairs, n)
    P = len(pairs)
    assert all(len(p.swords) == n and len(p.fwords) == n for p in pairs)
    assert P * n <= synth.VOCAB_SIZE
    script = np.random.default_rng(seed).permutation(synth.VOCAB_SIZE)[:P * n].astype(np.uint32)
    swords = [w for p in pairs for w in p.swords]
    fwords = [w for p in pairs for w in p.fwords]
    quoted = np.array([not p.name.startswith(UNQUOTED) for p in pairs], dtype=bool)
    tok = script.reshape(P, n)[quoted].reshape(-1).copy()
    off = np.concatenate([[0], np.cumsum(quoted * n)]).astype(np.uint64)
    keep = np.repeat(quoted, n)
    if layout == "own":
        strings, tok_str = fwords, np.arange(P * n, dtype=np.uint32)[keep]
    elif layout in ("vec", "vec_explicit"):
        strings = [""] * synth.VOCAB_SIZE
        for j, w in enumerate(fwords):
            strings[int(script[j])] = w
        tok_str = tok.copy() if layout == "vec_explicit" else None
    else:
        raise ValueError(layout)
    chars, coff = pack_strings(strings)
    lev = np.repeat(np.array([pair_distance(p) if q else 0 for p, q in zip(pairs, quoted)],
                             dtype=np.uint32), n)
    return Built(n, pairs, script, swords, tok, off, chars, coff, tok_str,
                 np.repeat(np.arange(P, dtype=np.uint32), n)[keep],
                 np.tile(np.arange(n, dtype=np.uint32), P)[keep],
                 np.arange(P * n, dtype=np.uint32)[keep], lev[keep])


def assert_predicted(rows, built):
    """The records of a search of `built` are the predicted ones: n per work, in order."""
    assert len(rows) == len(built.work), (len(rows), len(built.work))
    for name, want in (("work", built.work), ("fan_ix", built.fan_ix), ("orig_ix", built.orig_ix),
                       ("lev", built.lev)):
        bad = np.nonzero(rows[name] != want)[0]
        if bad.size:
            p = built.pairs[int(built.orig_ix[bad[0]]) // built.n]
            raise AssertionError("%s of record %d: %d, predicted %d; pair %r: script %r fan %r"
                                 % (name, int(bad[0]), int(rows[name][bad[0]]), int(want[bad[0]]), p.name,
                                    script_text(p)[:80], fan_text(p)[:80]))


@functools.lru_cache(maxsize=None)
def oracle_rows(name, layout):
    """(Built, rows of the C oracle) of a named case list, computed once per process."""
    from fandom_search_amd import abi
    n, pairs = cases(name)
    b = build(pairs, n, layout)
    want = oracle_search(b, abi.make_config(window_size=n))
    want.setflags(write=False)
    return b, want


def oracle_search(b, cfg):
    from oracle import c_oracle
    sch, so = pack_strings(b.swords)
    oi = c_oracle.OracleIndex(cfg, b.script, sch, so, synth.embedding(), synth.lsh_normals(b.n), threads=8)
    try:
        rows, _ = oi.search(b.tok, b.off, b.chars, b.coff, tok_str=b.tok_str)
    finally:
        oi.close()
    return rows
