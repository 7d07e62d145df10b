"""The LSH key signs restated in plain numpy (no GPU), and inputs whose float32 projection sums
cancel: test_keys_restated_host.py proves on the CPU that the inputs bite, test_gpu_hostile_keys.py
runs them on the device.

Canonical keys: A[k][v][c] by sequential multiply-add over d, p[c] in slot order in
float64, bit = p > 0; an out-of-vocabulary (OOV) id's row is the sum of the `nt` entries of its
distinct hot positions in a_value's order.  The float32 path as the kernels compute it
(fs_lsh.h: row32; lsh_window, k_lsh_batch, k_lsh_pkeys, k_lsh_scan): rows are float32(A), an OOV
row is the float32 sum of the float32(nt) rows (skipping b == a and c == b), the sum is taken in
slot order in float32.  A float32 sign is trusted when |sum| > bound (`decision_bound`, the
mirror of fs_lsh.h: key_bound32); a window with a column that is not redoes all its columns in
float64.

Per window and column a class (`classify`):
  AGREE      the float32 sign is the float64 sign
  ZERO       the float32 sum is 0 and the float64 sum is not
  FLIPPED    the float32 sum is not 0 and its sign bit differs from the float64 sum's
  NONFINITE  the float32 sum is inf or NaN (rows that overflow float32)

Hostile inputs (`make_case`).  `emb` and `normals` are both inputs, so a projection can be
planted exactly.  The table has G groups of four near-synonyms {on, off} x {+, -}:
  e = scale_e * [on * 2^-6, +-1/4, one-hot(group)]              (D = 16, G = 14, V = 56)
One *hostile column* c* has weights on the `on` channel only, 64 * x_k at slot k, so that a
window's projection on it is the sum of x_k over its `on` slots -- exactly, in float64.  Three
slots hold values near 1, -1/2, -1/2 with offsets of a fraction of a float32 spacing (found by
search, accepted by `classify`): windows with exactly those slots on are FLIPPED (float64 sum
> 0, float32 sum < 0); a fourth slot holds the value that makes {first, second, fourth} ZERO
(float64 sum > 0).  For an OOV case the three values sit on the three hot positions of one id
at one slot instead, so that the cancellation happens inside row32's float32 sum.
Every other column has weights on the group dimensions only (the same projection for all four
variants of a word), but for one *separator* column in every table other than c*'s: a weight
on the +- channel of slot m alone.

A planted fan window F differs from a script line S in slot m alone, by a near-synonym, so
their distance is far below the threshold:
  polarity 1   S = {hostile slots on; m off, +}   F = {the same; m off, -}: the same projection
               on c*; true bit equal to S's, float32 bit different: the record must exist
  polarity 2   S = {hostile slots on; m on, +}    F = {...; m off, -}: S's projection is
               x_m = -1/4 lower, robustly negative; true bit different from S's, float32 bit
               equal: the record must not exist
F and S share the bucket of c*'s table iff the bit of c* is equal, and no other table's (the
separators), so F's record exists iff the hostile bit is right.
"""

import zlib

import numpy as np

from fandom_search_amd import abi
from fandom_search_amd.vocab import pack_strings

U = 2.0 ** -24
AGREE, ZERO, FLIPPED, NONFINITE = 0, 1, 2, 3
D, G = 16, 14
V = 4 * G
SEP = 0.25                       # the +- channel
ON = 2.0 ** -6                   # the on channel: invisible to the cosines
THR = 0.05                       # F to S: 0.02 at n = 6; one unrelated slot: 0.094 at n = 10


# ---- the canonical tables and the float32 path ----------------------------------

def nt_of(normals, n, d):
    """nt[k][d][c] = normals[c][k * D + d] (k_nt)."""
    nm = np.asarray(normals, dtype=np.float64).reshape(-1, n, d)
    return np.ascontiguousarray(nm.transpose(1, 2, 0))


def a_tables(emb, normals, n):
    """A[k][v][c] = seqsum_d nt[k][d][c] * (double) E[v][d]: separate multiply and add, d ascending."""
    e = np.asarray(emb, dtype=np.float32).astype(np.float64)
    nt = nt_of(normals, n, e.shape[1])
    acc = np.zeros((n, e.shape[0], nt.shape[2]))
    for d in range(e.shape[1]):
        acc = acc + nt[:, None, d, :] * e[None, :, d, None]
    return acc


def oov_hot(tid, d):
    code = int(tid) & ~abi.FS_OOV_FLAG
    return code // (d * d), (code // d) % d, code % d


def oov_id(a, b, c, d=D):
    return abi.FS_OOV_FLAG | ((a * d + b) * d + c)


def round_up32(x):
    """__double2float_ru of |x|."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    low = f.astype(np.float64) < x
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


class Tables(object):
    """What the index holds for the keys: A and nt in float64, their float32 copies, and the
    rows' largest magnitudes rounded up (k_atab, k_nt32)."""

    def __init__(self, emb, normals, n):
        self.n, self.d = n, emb.shape[1]
        self.a = a_tables(emb, normals, n)
        self.nt = nt_of(normals, n, self.d)
        with np.errstate(over="ignore"):
            self.a32 = self.a.astype(np.float32)
            self.nt32 = self.nt.astype(np.float32)
        self.amax = round_up32(self.a).max(axis=2)
        self.ntmax = round_up32(self.nt).max(axis=2)

    def row64(self, k, tid):
        if not int(tid) & abi.FS_OOV_FLAG:
            return self.a[k, int(tid)]
        a, b, c = oov_hot(tid, self.d)
        acc = 0.0 + self.nt[k, a]
        if b != a:
            acc = acc + self.nt[k, b]
        if c != b:
            acc = acc + self.nt[k, c]
        return acc

    def row32(self, k, tid):
        if not int(tid) & abi.FS_OOV_FLAG:
            return self.a32[k, int(tid)]
        a, b, c = oov_hot(tid, self.d)
        with np.errstate(over="ignore", invalid="ignore"):
            r = self.nt32[k, a]
            if b != a:
                r = r + self.nt32[k, b]
            if c != b:
                r = r + self.nt32[k, c]
        return r

    def row_bound(self, k, tid):
        """row32_bound: (>= max_c |row|, float32 addends behind the row)."""
        if not int(tid) & abi.FS_OOV_FLAG:
            return self.amax[k, int(tid)], 1
        a, b, c = oov_hot(tid, self.d)
        m, terms = self.ntmax[k, a], 1
        if b != a:
            m, terms = np.float32(m + self.ntmax[k, b]), terms + 1
        if c != b:
            m, terms = np.float32(m + self.ntmax[k, c]), terms + 1
        return m, terms

    def projections(self, tok):
        """p64[w][c] and p32[w][c] of every window of the token stream `tok`, in slot order."""
        tok = np.asarray(tok)
        w = len(tok) - self.n + 1
        p64 = p32 = None
        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(self.n):
                r64 = np.stack([self.row64(k, t) for t in tok[k:k + w]])
                r32 = np.stack([self.row32(k, t) for t in tok[k:k + w]])
                p64 = r64 if k == 0 else p64 + r64
                p32 = r32 if k == 0 else p32 + r32
        assert p32.dtype == np.float32 and p64.dtype == np.float64
        return p64, p32

    def bounds(self, tok, slack=1.0):
        """The decision bound of every window (`decision_bound`)."""
        tok = np.asarray(tok)
        out = np.zeros(len(tok) - self.n + 1, dtype=np.float32)
        for w in range(len(out)):
            am, terms = np.float32(0.0), 0
            for k in range(self.n):
                m, t = self.row_bound(k, tok[w + k])
                am, terms = np.float32(am + m), terms + t
            out[w] = decision_bound(am, terms, self.n, slack)
        return out


def decision_bound(am, terms, n, slack=1.0):
    """fs_lsh.h: key_bound32.  The relative part, terms * 2^-22 * am, is four times the worst
    case of `terms` roundings to float32 of magnitude <= am in all and the additions behind them;
    the absolute part, terms * 2^-149, covers what a relative bound cannot: the rounding of a
    row below 2^-126 is up to 2^-150 whatever the row's size.  FS_LSH_F32_SLACK multiplies
    both (0: every float32 sum that is not 0 is trusted)."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        scale = np.float32(n * 2.0 ** -22 * slack)
        absolute = np.float32(2.0 ** -149 * slack)
        rel = np.float32(np.float32(scale * np.float32(am)) * np.float32(np.float32(terms) / np.float32(n)))
        return np.float32(rel + np.float32(absolute * np.float32(terms)))


def classify(p64, p32):
    with np.errstate(invalid="ignore"):
        out = np.full(p64.shape, AGREE, dtype=np.int8)
        out[(p32 == 0) & (p64 != 0)] = ZERO
        out[(p32 != 0) & ((p32 > 0) != (p64 > 0))] = FLIPPED
        out[~np.isfinite(p32)] = NONFINITE
    return out


def keys_of(bits, h, b):
    """key h of every window from its column bits: column h * B + j is bit j of the key string,
    the first column the most significant (RandomBinaryProjections.hash_vector)."""
    w = bits.shape[0]
    v = bits.reshape(w, h, b).astype(np.uint64)
    weights = (np.uint64(1) << np.arange(b - 1, -1, -1, dtype=np.uint64))
    return (v * weights[None, None, :]).sum(axis=2).astype(np.uint32)


def bits64(p64):
    return p64 > 0


def bits32(p32):
    with np.errstate(invalid="ignore"):
        return p32 > 0


def bits_decided(p64, p32, bound):
    """What the kernels give: the float32 signs of a window whose columns are all farther from
    zero than its bound, the float64 signs of every other window."""
    with np.errstate(invalid="ignore"):
        sure = (np.abs(p32) > bound[:, None]).all(axis=1)
    return np.where(sure[:, None], bits32(p32), bits64(p64))


# ---- hostile inputs ------------------------------------------------------------

def half_spacing(exp):
    """Half a float32 spacing at 2^exp, relative to 2^exp."""
    return max(2.0 ** -24, 2.0 ** (-150 - exp))


def find_offsets(exp, order):
    """Values x1 ~ 1, x2 ~ -1/2, x3 ~ -1/2 (FLIPPED: float64 sum > 0, float32 sum < 0 at scale
    2^exp) and xz ~ -1/2 ({x1, x2, xz} ZERO: float32 sum 0, float64 sum > 0), offsets in 64ths of
    half a spacing; `order` is the order in which the slots that hold (x1, x2, x3, xz) are
    summed.  Found by search, accepted by `classify`."""
    r = half_spacing(exp) / 64.0
    s = 2.0 ** exp

    def cls(vals, pos):
        v = np.array([x for _, x in sorted(zip(pos, vals))]) * s
        p32 = np.float32(0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            f = v.astype(np.float32)
            p32 = f[0]
            for x in f[1:]:
                p32 = np.float32(p32 + x)
        p64 = 0.0
        for i, x in enumerate(v):
            p64 = x if i == 0 else p64 + x
        return int(classify(np.array([p64]), np.array([p32], dtype=np.float32))[0]), p64, p32

    rng = np.random.default_rng(12345)
    for _ in range(20000):
        a, b, c, z = (int(t) for t in rng.integers(-127, 128, size=4))
        x = [1.0 + a * r, -(0.5 + b * r), -(0.5 + c * r)]
        xz = -(0.5 + z * r)
        k1, p1, q1 = cls(x, order[:3])
        k2, p2, q2 = cls([x[0], x[1], xz], [order[0], order[1], order[3]])
        if k1 == FLIPPED and p1 > 0 and q1 < 0 and k2 == ZERO and p2 > 0:
            return x + [xz]
    raise AssertionError("no offsets found at 2^%d" % exp)


SLOTS = {
    # name: (slots of x1, x2, x3, xz, m) as functions of n
    "head": lambda n: (0, 1, 2, 3, n - 1),          # the cancelling slots 0 and 1
    "tail": lambda n: (n - 1, n - 2, n - 3, n - 4, 0),   # the last two slots
    "span": lambda n: (0, n - 1, n - 2, 1, 3),      # the first slot against the last two
}


def make_case(n=6, h=8, b=8, hcol=0, slots="head", oov=False, exp_e=0, exp_n=0, seed=1,
              per_kind=4, n_works=4, nearest=10, unique=1, small=False, generic=2.0 ** -5, tiny=0):
    """The inputs of one case and what was planted.  `hcol`: the hostile column (-1: the last);
    `exp_e`, `exp_n`: emb and normals times 2^exp; `small`: a short script and short works (wide
    buckets, C = 1); `generic`: the size of the other columns' weights; `tiny`: the rows of the
    second half of the groups times 2^tiny (float32-subnormal table rows next to ordinary ones),
    the planted lines and the works made of those rows, the script's filler of ordinary ones."""
    rng = np.random.default_rng(seed)
    c_all = h * b
    hcol = hcol % c_all
    htab = hcol // b
    i1, i2, i3, iz, m = SLOTS[slots](n)
    se, sn = 2.0 ** exp_e, 2.0 ** exp_n

    emb = np.zeros((V, D))
    for g in range(G):
        for on in (0, 1):
            for sb in (0, 1):
                v = 4 * g + 2 * on + sb
                emb[v, 0] = on * ON
                emb[v, 1] = SEP if sb == 0 else -SEP
                emb[v, 2 + g] = 1.0
    emb[V // 2:] *= 2.0 ** tiny
    emb = (emb * se).astype(np.float32)

    normals = np.zeros((c_all, n, D))
    normals[:, :, 2:] = rng.standard_normal((c_all, n, D - 2)) * generic
    normals[hcol] = 0.0
    seps = []
    for t in range(h):
        if t != htab:
            c = t * b + b - 1
            seps.append(c)
            normals[c] = 0.0
            normals[c, m, 1] = 1.0
    overflow = exp_e + exp_n > 100                 # (rows beyond float32: the offsets of scale 1)
    x = find_offsets(0 if overflow else exp_e + exp_n + tiny, (0, 1, 2, 3) if oov else (i1, i2, i3, iz))
    oov_slot = i1
    ids = {}
    if oov:
        # the three values on the hot positions of one id at slot `oov_slot`; a fourth position
        # for the ZERO id, a fifth for the id with two coinciding positions (two addends: ZERO)
        normals[hcol, oov_slot, 3], normals[hcol, oov_slot, 7], normals[hcol, oov_slot, 11] = x[0], x[1], x[2]
        normals[hcol, oov_slot, 12] = x[3]
        normals[hcol, oov_slot, 13] = -(x[0] - 0.125 * U)
        ids = dict(flip=oov_id(3, 7, 11), zero=oov_id(3, 7, 12), two=oov_id(3, 3, 13),
                   quiet=oov_id(4, 8, 14))           # (`quiet`: a second OOV token, 0 on c*)
    else:
        for slot, val in zip((i1, i2, i3, iz), x):
            normals[hcol, slot, 0] = val / ON
    normals[hcol, m, 0] = -0.25 / ON
    normals = (normals * sn).reshape(h, b, n * D)

    def word(g, on, sb):
        return 4 * g + 2 * on + sb

    # the kinds of planted windows: (class, polarity, OOV ids of the line)
    if oov:
        kinds = [(FLIPPED, 1, ("flip",)), (FLIPPED, 2, ("flip",)), (FLIPPED, 1, ("flip", "quiet")),
                 (FLIPPED, 2, ("flip", "quiet")), (ZERO, 1, ("zero",)), (ZERO, 2, ("zero",)),
                 (ZERO, 1, ("two",)), (ZERO, 2, ("two", "quiet"))]
        per_kind = max(1, per_kind // 2)
    else:
        kinds = [(FLIPPED, 1, ()), (FLIPPED, 2, ()), (ZERO, 1, ()), (ZERO, 2, ())]
    lines = []
    for kind, pol, oo in kinds:
        for _ in range(per_kind):
            groups = rng.integers(G // 2 if tiny else 0, G, size=n)
            on = np.zeros(n, dtype=int)
            if not oov:
                on[[i1, i2, i3 if kind == FLIPPED else iz]] = 1
            s_line = [word(int(groups[k]), int(on[k]), int(rng.integers(0, 2))) for k in range(n)]
            f_line = list(s_line)
            s_line[m] = word(int(groups[m]), 1 if pol == 2 else 0, 0)
            f_line[m] = word(int(groups[m]), 0, 1)
            if oo:
                s_line[oov_slot] = f_line[oov_slot] = ids[oo[0]]
                if len(oo) > 1:
                    s_line[i2] = f_line[i2] = ids[oo[1]]
            lines.append((kind, pol, s_line, f_line))

    def filler(k, fan):
        # (the script's filler from the first half of the groups, the works' from the second: a
        # window that overlaps a planted one has no script window within the threshold)
        return [int(t) + (V // 2 if fan else 0) for t in rng.integers(0, V // 2, size=k)]

    script, s_at = filler(3, False), []
    for _, _, s_line, _ in lines:
        s_at.append(len(script))
        script += s_line + filler(2 if small else 3, False)
    works = [filler(4, True) for _ in range(n_works)]
    planted = []
    for j in rng.permutation(len(lines)):
        kind, pol, _, f_line = lines[j]
        w = int(np.argmin([len(x) for x in works]))
        planted.append(dict(work=w, fan_ix=len(works[w]), orig_ix=s_at[j], polarity=pol,
                            kind=NONFINITE if overflow else kind))
        works[w] += f_line + filler(n + 1 if small else n + 4, True)
    off = np.zeros(n_works + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in works])
    for p in planted:
        p["pos"] = int(off[p["work"]]) + p["fan_ix"]
    script = np.asarray(script, dtype=np.uint32)
    tok = np.asarray([t for x in works for t in x], dtype=np.uint32)
    oov_ids = sorted(set(ids.values()))
    strings = ["w%d" % v for v in range(V)] + ["oov%d" % i for i in range(len(oov_ids))]

    def str_id(t):
        return V + oov_ids.index(int(t)) if int(t) & abi.FS_OOV_FLAG else int(t)

    chars, coff = pack_strings(strings)
    cfg = abi.make_config(window_size=n, number_of_hashes=h, hash_dimensions=b, distance_threshold=THR,
                          emb_dim=D, nearest_n=nearest, unique_filter=unique, mode=abi.FS_MODE_AUTO)
    return dict(cfg=cfg, n=n, h=h, b=b, hcol=hcol, seps=seps, emb=emb, normals=normals, script=script,
                swords=[strings[str_id(t)] for t in script], tok=tok,
                tok_str=np.asarray([str_id(t) for t in tok], dtype=np.uint32), off=off, chars=chars,
                coff=coff, strings=strings, planted=planted, overflow=overflow, exp=exp_e + exp_n + tiny)


def case_keys(case, slack=1.0):
    """Per window of the fan token stream: the classes, and the keys in float64, in float32 and as
    decided at `slack`; the script windows' keys in float64.  (Windows across a work boundary are
    included: nobody looks them up.)"""
    t = Tables(case["emb"], case["normals"].reshape(case["h"] * case["b"], -1), case["n"])
    p64, p32 = t.projections(case["tok"])
    s64, _ = t.projections(case["script"])
    hb = (case["h"], case["b"])
    bound = t.bounds(case["tok"], slack)
    return dict(cls=classify(p64, p32), p64=p64, p32=p32, bound=bound,
                k64=keys_of(bits64(p64), *hb), k32=keys_of(bits32(p32), *hb),
                kdec=keys_of(bits_decided(p64, p32, bound), *hb),
                script=keys_of(bits64(s64), *hb))


def assert_planted(case, keys=None):
    """The condition of every case, from the restatement: at least 8 FLIPPED and 8 ZERO planted
    windows on the hostile column (16 NONFINITE where the rows overflow float32), the true bit 1,
    every other column of a planted window AGREE and not 0 in float32 (so that a bound of 0 trusts
    a FLIPPED window), and, at scale 1, a FLIPPED float32 sum above 1/256 of the window's bound:
    a bound 256 times too tight trusts it.  (The bound is 4 n 2^-24 am with am >= 2 here and the
    sum one or two spacings of 2^-24: 100 times would not do at n = 10.)"""
    keys = keys or case_keys(case)
    hc = case["hcol"]
    count = {FLIPPED: 0, ZERO: 0, NONFINITE: 0}
    for p in case["planted"]:
        w = p["pos"]
        cls = keys["cls"][w]
        assert keys["p64"][w, hc] > 0
        others = np.delete(np.arange(cls.shape[0]), hc)
        if case["overflow"]:
            assert cls[hc] == NONFINITE
        else:
            assert cls[hc] == p["kind"], (p, cls[hc])
            assert (cls[others] == AGREE).all() and (keys["p32"][w, others] != 0).all(), p
            if p["kind"] == FLIPPED and case["exp"] == 0:
                assert float(keys["bound"][w]) < 256.0 * abs(float(keys["p32"][w, hc])), p
        count[int(cls[hc])] += 1
    if case["overflow"]:
        assert count[NONFINITE] >= 16
    else:
        assert count[FLIPPED] >= 8 and count[ZERO] >= 8, count
    return count


def planted_words(case, kinds=(FLIPPED, ZERO)):
    """(work, fan_ix) of every word of the planted windows of the given kinds."""
    return {(p["work"], p["fan_ix"] + k) for p in case["planted"] if p["kind"] in kinds
            for k in range(case["n"])}


def differing_words(a, b):
    """(work, fan_ix) of the records that one of two record arrays has and the other has not, or
    has differently."""
    def as_set(rows):
        return {(int(r["work"]), int(r["fan_ix"]), int(r["orig_ix"]), int(r["lev"]),
                 float(r["dist"]).hex(), float(r["comb"]).hex()) for r in rows}
    return {(t[0], t[1]) for t in as_set(a) ^ as_set(b)}


# ---- the cases of test_gpu_hostile_keys.py ----------------------------------------

LEV_LANE = {"FS_LSH_LEV_LANE": "2"}      # the deferred forms (k_lsh_batch, k_lsh_pkeys) however few windows are pending


def _env(**kw):
    return dict(LEV_LANE, **kw)


# The four places where the decision is written out, by the switches that reach them.
# name: (environment, kernels that must be launched, kernels that must not be)
SITES = {
    "verify": (_env(FS_LSH_BATCH="0"), ("k_lsh_verify",), ("k_lsh_batch", "k_lsh_pkeys", "k_lsh_scan")),
    "verify_serial": (_env(FS_LSH_SERIAL="1"), ("k_lsh_verify",), ("k_lsh_batch", "k_lsh_pkeys", "k_lsh_scan")),
    "batch": (_env(FS_LSH_EMAP="0"), ("k_lsh_batch",), ("k_lsh_verify", "k_lsh_pkeys", "k_lsh_scan")),
    "batch_unfused": (_env(FS_LSH_EMAP="0", FS_NEAR_FUSED="0"), ("k_lsh_batch",),
                      ("k_lsh_verify", "k_lsh_pkeys", "k_lsh_scan", "k_near_sift")),
    "pkeys": (_env(), ("k_lsh_pkeys", "k_lsh_enum"), ("k_lsh_verify", "k_lsh_scan")),
    "scan": (_env(FS_LSH_PREFILTER="0", FS_LSH_SHARE="0"), ("k_lsh_scan",), ("k_share", "k_near_sift")),
    "scan_verify": (_env(FS_LSH_PREFILTER="0", FS_LSH_BATCH="0"), ("k_lsh_scan", "k_lsh_verify"),
                    ("k_near_sift", "k_lsh_batch")),
}
MAIN_SITES = ("verify", "batch", "pkeys", "scan")

# name: make_case arguments.  C = h * b; hcol: the hostile column.
CASES = {
    "base": dict(n=6, h=8, b=8, hcol=3),
    # the hostile column: 0, 3, 4 and C - 1; C = 150: the last lane holds 2 live columns and 2
    # padded ones; C = 255, 256: the widest the float32 path takes; C = 272: the float64-only
    # control (k_lsh_scan takes a second round of 256 columns there)
    "c1": dict(n=6, h=1, b=1, hcol=0, small=True),
    "c150_col0": dict(n=6, h=15, b=10, hcol=0),
    "c150_col3": dict(n=6, h=15, b=10, hcol=3),
    "c150_col4": dict(n=6, h=15, b=10, hcol=4),
    "c150_col148": dict(n=6, h=15, b=10, hcol=148),
    "c150_last": dict(n=6, h=15, b=10, hcol=-1),
    "c255_last": dict(n=6, h=15, b=17, hcol=-1),
    "c256_last": dict(n=6, h=16, b=16, hcol=-1),
    "c256_col252": dict(n=6, h=16, b=16, hcol=252),
    "c272_last": dict(n=6, h=16, b=17, hcol=-1),
    "h1_b12": dict(n=6, h=1, b=12, hcol=4),
    # the cancelling slots: 0 and 1, the last two, the first against the last two; n = 10 loads
    # its rows in two groups of eight in lsh_window and takes one window at a time in k_lsh_batch
    "n6_tail": dict(n=6, h=8, b=8, hcol=3, slots="tail"),
    "n6_span": dict(n=6, h=8, b=8, hcol=4, slots="span"),
    "n8_head": dict(n=8, h=8, b=8, hcol=0, slots="head"),
    "n8_tail": dict(n=8, h=8, b=8, hcol=-1, slots="tail"),
    "n10_head": dict(n=10, h=8, b=8, hcol=3, slots="head"),
    "n10_tail": dict(n=10, h=8, b=8, hcol=4, slots="tail"),
    "n10_span": dict(n=10, h=8, b=8, hcol=-1, slots="span"),
    # scale: projections in the float32 subnormal range; rows that overflow float32.  (Nine bits
    # are left of a float32 at 2^-140: the other columns get weights of the hostile column's size
    # there, and the seed is one that leaves them AGREE on the planted windows.)
    "subnormal": dict(n=6, h=3, b=4, hcol=3, exp_e=-40, exp_n=-100, generic=1.0),
    "subnormal_n10": dict(n=10, h=3, b=6, hcol=-1, exp_e=-40, exp_n=-100, slots="span", generic=1.0),
    "overflow": dict(n=6, h=3, b=4, hcol=3, exp_e=40, exp_n=100),
    # one table that mixes float32-subnormal rows (2^-134; the planted lines and the works) with
    # ordinary ones (the script's filler) under ordinary normals
    "mixed": dict(n=6, h=3, b=4, hcol=3, tiny=-134, generic=1.0),
}
# OOV windows: the hostile sum is row32's (one id with three distinct hot positions; an id with
# two coinciding positions; two OOV tokens in a window: 8, 7 and 10 float32 addends at n = 6)
OOV_CASES = {
    "oov": dict(n=6, h=8, b=8, hcol=3, oov=True),
    "oov_n8_last": dict(n=8, h=15, b=10, hcol=-1, oov=True),
}
# (a script with OOV tokens has no component prefilter: k_lsh_scan or the share rule flags the
# windows, k_lsh_batch or k_lsh_verify takes them; 64: float64 for OOV windows)
OOV_ENVS = {
    "default": _env(),
    "noshare": _env(FS_LSH_SHARE="0"),
    "verify": _env(FS_LSH_SHARE="0", FS_LSH_BATCH="0"),
    "diag64": _env(FS_LSH_DIAG="64"),
    "diag64_noshare": _env(FS_LSH_DIAG="64", FS_LSH_SHARE="0"),
}

_CACHE = {}


def case(name):
    """A case by name, made once (its inputs are not changed by anyone)."""
    if name not in _CACHE:
        kw = CASES.get(name) or OOV_CASES[name]
        seed = zlib.crc32(name.encode()) & 0xFFFF
        for _ in range(64):                  # (the first seed whose planted windows are as `assert_planted` asks)
            made = make_case(seed=seed, **kw)
            try:
                assert_planted(made)
                break
            except AssertionError:
                seed += 1000
        _CACHE[name] = made
    return _CACHE[name]
