"""The share rule (csrc/fs_lsh_share.hip, index side fs_build_share in csrc/fs_lsh_build.hip) restated
in plain Python, and window pairs built at its bounds: test_share_bounds_host.py proves on the CPU,
in exact arithmetic, that the pairs lie where they should and that the restated rule is sound on
them; test_gpu_share_bounds.py runs the kernels on the same pairs.

The rule (`Rule`).  tau = 1 - thr - 1e-6, phi = (1 - tau^2) / (1 - gamma^2), share_lim =
float32((1 - phi)(1 - 1e-6)), share_scale = 2^20 / max(norm_max^2 (1 + 1e-9), 3).
  asks           the gate, run by run (share_blocks / share_block_start restated from fs_hash.h):
                 integer shares qi = floor(q * share_scale), per run the float32 threshold
                 floorf(share_lim * all) - base - (K1 - K0) - 2 (base: qi + 1 of every slot that
                 agrees with anything), the subsets of the run's usable slots that reach it and
                 stop reaching it without their smallest slot.  None: the window is not
                 constrained (a run whose threshold is not positive, or more than kEnumCap masks).
  pair_possible  the pairs' test: A from the fan side, the exit at A >= phi (1 + 1e-9), then B and
                 sqrt((1-A)(1-B)) + gamma sqrt(AB) > tau.
The restated rule takes true component ids; the kernels' pairs' test compares a few hash bits of
them and can only find fewer far slots.  They may flag more windows, never fewer records.

More than kEnumCap masks cannot happen for windows of up to twelve slots: the masks a run asks for
are an antichain (no mask contains another: a mask leaves the list when its smallest slot can go),
so a run of r slots asks for at most C(r, r // 2) of them -- 20 for six slots, 10 + 10 for ten,
18 for twelve.  The `cnt > cap` outcome is restated as the kernel has it; `cap_windows` builds the
windows that reach exactly 20 (six near-equal shares; ten slots in two runs of five, where the
limit lies between two and three fifths), and test_share_bounds_host.py asserts that nothing
passes 20.

The table (`Bounds`): float32, emb_dim 64, a few hundred rows, every row a multiple of a
*direction*; the directions are rows of the 64 x 64 Hadamard matrix over 8 (orthonormal, every
coordinate +-1/8: sqrt(3) max|u_d| / |u| = 0.217, so the index proves out-of-vocabulary fan tokens
far from every row) or, for a twin, c h_a + sqrt(1 - c^2) h_b:
  g0 .. g16      parallel groups: rows of one direction with different norms (cosine 1, one
                 component) -- an agreeing slot carries another norm on either side
  u_t / v_t      borderline twins, cosine gamma - 1.2e-4, gamma - 2e-4, gamma - 1e-3: far, just
                 under the gamma - 1e-4 that k_near_pairs applies in float32; nothing links them
  nu_t / nv_t    near twins, cosine gamma + 1e-3: one component
  sf_i / ff_i    filler of the script and of the fan text, orthogonal to all of the above
  two zero rows  near nothing: a component each
A window pair (F, S) with far set Dm: agreeing slots hold rows of one group on either side, norms
in the ratio 1 : 1.25 throughout; far slots hold u_t on the fan side and v_t on the script side,
squared norms A / (1 - A) and B / (1 - B) of the agreeing slots', A = phi - delta,
B = gamma^2 A / ((1 - A) + gamma^2 A) (the B that maximises the bound).  Both Cauchy-Schwarz steps
are then tight: cos(F, S) = sqrt((1-A)(1-B)) + c sqrt(AB), c the twin's cosine.  Above six slots
A is the far share of the *runs that hold far slots*; in the families whose far slots leave a run
without one, that run's rows are 64 times shorter (a 4096th of the squared norm), so that the
window's far share is phi - delta to within 2e-4 as well.  Pair j takes group (a_j k + b_j) mod 17
in slot k: two pairs share at most one agreeing slot, so F_j is near S_j alone.

Families, each over LADDER (delta from 1e-2 through the boundary to -1e-3):
  pos_k          one far slot, at every position k (twin k mod 3: the closest records are at
                 k = 0 mod 3)
  in_run         two far slots inside one run
  two_runs       (n >= 7) a far slot in each of two runs
  every_run      (n >= 11) a far slot in each of the three runs
  all_of_run_r   (n >= 7) the far set is run r; the other runs agree, their last slot so heavy that
                 every mask asked for holds it (for nine slots: bit 8)
  wild2          an agreeing slot holds a fan name with two distinct hot positions (it agrees with
                 anything: the `base` term, with a small share -- where the script holds a name,
                 which the index allows for gamma >= 0.668; at gamma 0.5 only with FS_LSH_SHARE=43)
  name3          ... a fan name with three (far from everything; agrees with anything in an index
                 built with FS_LSH_SHARE=43)
  zero_agree / zero_far   a zero row in an agreeing slot (the same row) / in a far slot (the other)
and without a ladder: wild_large (the two-position name holds the largest share: the threshold is
not positive, the window is not constrained), all_wild_r (run r is names with two positions: not
constrained; above six slots a record all the same, the other runs agree), cap (above).

Closeness of the closest record per family, over n = 6 .. 12 and (thr, gamma) = (0.1, 0.7),
(0.05, 0.85), (0.25, 0.5), as test_share_bounds_host.py measures and asserts (both at most 2e-3):
the closest record being the one nearest phi among those whose far run is heavy by itself; the
ranges are over the 21 (n, configuration):
  family       (phi - A) / phi       (agreeing integer sum - thr) / thr, in the run at its bound
  pos          1.7e-4 .. 8.9e-4      5.3e-6 .. 4.7e-4
  in_run       1.7e-4 .. 1.3e-3      8.3e-6 .. 4.7e-4
  two_runs     1.7e-4 .. 9.8e-4      1.6e-4 .. 4.7e-4
  every_run    1.7e-4 .. 8.5e-4      2.5e-4 .. 4.7e-4
  all_of_run   1.7e-4 .. 8.5e-4      --
  wild2        2.2e-4 .. 1.4e-3      1.9e-5 .. 7.8e-4
  name3        2.0e-4 .. 1.6e-3      0 .. 7.7e-4
  zero_agree   1.7e-4 .. 1.1e-3      7.2e-6 .. 4.7e-4
  zero_far     1.6e-4 .. 1.2e-3      8.4e-6 .. 4.7e-4
all_of_run has the first only: its far run holds no agreeing slot and the other runs agree in
full, so no run of it can be near its integer threshold (sum / thr is 1 / lim there).
"""

import math
from fractions import Fraction

import numpy as np

K_ENUM_CAP = 20
OOV_FLAG = 0x80000000
WILD, NONE = -1, -2                    # a fan token that agrees with anything / with nothing
D = 64
CONFIGS = ((0.1, 0.7), (0.05, 0.85), (0.25, 0.5))           # (distance_threshold, FS_SHARE_GAMMA)
SIZES = (6, 7, 8, 9, 10, 11, 12)
LADDER = (1e-2, 1e-3, 5e-4, 3e-4, 2e-4, 1e-4, 0.0, -1e-3)
TWINS = (1.2e-4, 2e-4, 1e-3)           # gamma minus these: far
NEAR = 1e-3                            # gamma plus this: near
LAMBDA = 1.25                          # script norm over fan norm in an agreeing slot
SHORT = 1.0 / 64.0                     # the rows of a run that holds no far slot
PALETTE = (160.0, 176.0, 208.0, 224.0, 256.0)
GROUPS = 17
SH = 60                                # every float32 entry of the table times 2^SH is an integer


# ---- the rule ------------------------------------------------------------------------

def share_blocks(n):
    return 1 if n <= 6 else 2 if n <= 10 else 3


def share_block_start(n, r):
    b = share_blocks(n)
    if r <= 0:
        return 0
    if r >= b:
        return n
    if b == 2:
        return (n + 1) // 2
    return (n + 2) // 3 if r == 1 else (n + 2) // 3 + (n + 1) // 3


def runs_of(n):
    return [(share_block_start(n, r), share_block_start(n, r + 1)) for r in range(share_blocks(n))]


class Rule(object):
    def __init__(self, thr, gamma, norm_max):
        self.thr, self.gamma = float(thr), float(gamma)
        self.tau = 1.0 - self.thr - 1e-6
        self.phi = (1.0 - self.tau * self.tau) / (1.0 - self.gamma * self.gamma)
        self.lim = np.float32((1.0 - self.phi) * (1.0 - 1e-6))
        self.scale = 2.0 ** 20 / max(norm_max * norm_max * (1.0 + 1e-9), 3.0)

    def shares(self, q):
        return [int(x * self.scale) for x in q]

    def run_threshold(self, qi, wild, k0, k1):
        total = sum(qi[k0:k1])
        base = sum(qi[k] + 1 for k in range(k0, k1) if wild[k])
        return int(math.floor(float(self.lim * np.float32(total)))) - base - (k1 - k0) - 2

    def asks(self, qi, wild, usable, n, cap=K_ENUM_CAP):
        """The masks a fan window asks for, or None: not constrained."""
        masks = []
        for k0, k1 in runs_of(n):
            thr = self.run_threshold(qi, wild, k0, k1)
            if thr <= 0:
                return None
            for sub in range(1, 1 << (k1 - k0)):
                ks = [k0 + i for i in range(k1 - k0) if sub >> i & 1]
                if not all(usable[k] for k in ks):
                    continue
                s = sum(qi[k] for k in ks)
                if s >= thr and s - min(qi[k] for k in ks) < thr:
                    masks.append(sub << k0)
        return None if len(masks) > cap else set(masks)

    def pair_possible(self, far_mask, q_fan, q_script):
        n = len(q_fan)
        ff = af = 0.0
        for k in range(n):
            ff += q_fan[k]
            if far_mask >> k & 1:
                af += q_fan[k]
        if not ff > 0.0 or far_mask == 0:
            return True
        if af >= self.phi * (1.0 + 1e-9) * ff:
            return False
        A = min(af / ff, 1.0)
        bs = 0.0
        for k in range(n):
            if far_mask >> k & 1:
                bs += q_script[k]
        ss = 0.0
        for k in range(n):
            ss += q_script[k]
        if not ss > 0.0:
            return True
        B = min(bs / ss, 1.0)
        return math.sqrt((1.0 - A) * (1.0 - B)) + self.gamma * math.sqrt(A * B) > self.tau


def oov_code(a, b, c):
    return OOV_FLAG | ((a * D + b) * D + c)


def oov_hot(tok):
    code = tok & ~OOV_FLAG
    return sorted({code // (D * D), (code // D) % D, code % D})


# ---- the table and the pairs -------------------------------------------------------------

def hadamard():
    h = np.array([[1.0]])
    while len(h) < D:
        h = np.block([[h, h], [h, -h]])
    return h / 8.0


class Pair(object):
    """A planted window pair: fan and script tokens, the slots that differ in component."""
    def __init__(self, family, delta, fan, script, twin):
        self.family, self.delta, self.fan, self.script, self.twin = family, delta, list(fan), list(script), twin
        self.s_at = self.work = self.f_at = self.stream_at = None     # where the texts hold it

    def __repr__(self):
        return "%s delta=%g" % (self.family, self.delta)


class Bounds(object):
    """Table, script and fan text of one (n, thr, gamma)."""

    def __init__(self, n, thr, gamma, fan_stride=None, seed=7):
        self.n, self.thr, self.gamma = n, thr, gamma
        # a name in the script (its filler): only then does share_comp tell names with fewer than three
        # hot positions from the others -- and the index needs gamma >= 0.668 for such a script
        self.script_names = gamma >= 0.668
        self.runs = runs_of(n)
        H = hadamard()
        self.dirs, self.label = {}, {}
        at = 0
        for i in range(GROUPS):
            self.dirs["g%d" % i] = H[at]; at += 1
        self.twin_cos = []
        for t, d in enumerate(TWINS + (-NEAR, -NEAR)):
            c = gamma - d
            a, b = H[at], H[at + 1]; at += 2
            far = t < len(TWINS)
            nu, nv = ("u%d" % t, "v%d" % t) if far else ("nu%d" % (t - len(TWINS)), "nv%d" % (t - len(TWINS)))
            self.dirs[nu], self.dirs[nv] = a, c * a + math.sqrt(1.0 - c * c) * b
            if far:
                self.twin_cos.append(c)
            else:
                self.label[nu] = self.label[nv] = "n%d" % (t - len(TWINS))     # near: one class
        self.n_fill = (D - at) // 2
        for i in range(self.n_fill):
            self.dirs["sf%d" % i] = H[at]; at += 1
        for i in range(self.n_fill):
            self.dirs["ff%d" % i] = H[at]; at += 1
        self.rows, self.row_dir, self.row_id = [], [], {}
        self.zero = [self._row(None, 0.0, "z0"), self._row(None, 0.0, "z1")]
        rule0 = Rule(thr, gamma, 1.0)                 # (phi only: the scale waits for the table)
        self.phi = rule0.phi
        self.pairs = []
        self._families()
        # (planted windows far enough apart that a sub-tile's keys and list entries find room in
        # k_share_scan's lists: a window without room is flagged as it is, which the rule here does
        # not restate)
        self._texts(fan_stride or (52 if n <= 10 else 112), seed)
        self.emb = np.ascontiguousarray(np.stack(self.rows), dtype=np.float32)
        # squared norms as k_rownorms sums them: float64, coordinate by coordinate
        self.q = []
        for row in self.emb:
            acc = 0.0
            for x in row:
                acc += float(x) * float(x)
            self.q.append(acc)
        self.rule = Rule(thr, gamma, math.sqrt(max(self.q)))

    # -- rows
    def _row(self, d, norm, key=None):
        key = key or (d, float(np.float32(norm)))
        if key not in self.row_id:
            self.row_id[key] = len(self.rows)
            v = np.zeros(D) if d is None else self.dirs[d] * norm
            self.rows.append(v.astype(np.float32))
            self.row_dir.append(key if d is None else self.label.get(d, d))
        return self.row_id[key]

    # -- window pairs
    def _pair(self, family, delta, far, twin=0, short_runs=True, swaps=(), heavy_last=False, norms=None):
        """far: the far slots.  swaps: {slot: (fan token, script token)} put in afterwards, the
        slot taken out of the agreeing mass beforehand (a zero row, a name)."""
        n, j, swaps = self.n, len(self.pairs), dict(swaps)
        a, b = 1 + (j // GROUPS) % (GROUPS - 1), j % GROUPS
        far_runs = [r for r, (k0, k1) in enumerate(self.runs) if any(k0 <= k < k1 for k in far)]
        whole = [r for r in far_runs if all(k in far for k in range(*self.runs[r]))]
        fan, script = [None] * n, [None] * n
        mass = [0.0] * len(self.runs)                 # agreeing squared norm of the fan side, per run
        for r, (k0, k1) in enumerate(self.runs):
            short = SHORT if (short_runs and far_runs and r not in far_runs and not whole) else 1.0
            for k in range(k0, k1):
                if k in far or k in swaps:
                    continue
                p = PALETTE[(k + j) % len(PALETTE)]
                if heavy_last:
                    p = 256.0 if k == k1 - 1 else 64.0
                if norms is not None:
                    p = norms[k]
                p *= short
                g = "g%d" % ((a * k + b) % GROUPS)
                fan[k], script[k] = self._row(g, p), self._row(g, p * LAMBDA)
                mass[r] += float(np.float32(p)) ** 2
        A = self.phi - delta
        B = self.gamma ** 2 * A / ((1.0 - A) + self.gamma ** 2 * A)
        for r in far_runs:
            k0, k1 = self.runs[r]
            mine = [k for k in far if k0 <= k < k1]
            m = sum(mass) if whole else mass[r]       # (a whole run far: the window's share)
            qf = A / (1.0 - A) * m / len(mine)
            qs = B / (1.0 - B) * LAMBDA ** 2 * m / len(mine)
            for k in mine:
                fan[k] = self._row("u%d" % twin, math.sqrt(qf))
                script[k] = self._row("v%d" % twin, math.sqrt(qs))
        for k, (f, s) in swaps.items():
            fan[k], script[k] = f, s
        p = Pair(family, delta, fan, script, twin)
        self.pairs.append(p)
        return p

    def _families(self):
        n, runs = self.n, self.runs
        two = oov_code(3, 3, 9)                       # a name with two distinct hot positions
        three = oov_code(5, 17, 40)
        for k in range(n):
            for d in LADDER:
                self._pair("pos_%d" % k, d, [k], twin=k % 3)
        k0, k1 = runs[-1]
        for d in LADDER:
            self._pair("in_run", d, [k0, k1 - 1])
        if len(runs) >= 2:
            for d in LADDER:
                self._pair("two_runs", d, [runs[0][0] + 1, runs[-1][1] - 2])
        if len(runs) >= 3:
            for d in LADDER:
                self._pair("every_run", d, [k0 + 1 for k0, _ in runs])
        if len(runs) >= 2:
            for r in sorted({0, len(runs) - 1}):
                for d in LADDER:
                    self._pair("all_of_run_%d" % r, d, list(range(*runs[r])), heavy_last=True)
        k0, k1 = runs[0]
        small = self._row("g0", 2.0)
        for d in LADDER:
            self._pair("wild2", d, [k0], swaps={k0 + 2: (two, small)})
            self._pair("name3", d, [k0], swaps={k0 + 2: (three, small)})
            self._pair("zero_agree", d, [k0 + 1], swaps={k0 + 2: (self.zero[0], self.zero[0])})
            self._pair("zero_far", d, [k0 + 1], swaps={k0 + 2: (self.zero[0], self.zero[1])})
        # the name holds the largest share of its window: every row shorter than sqrt(2)
        self._pair("wild_large", 1e-2, [k0], swaps={k0 + 1: (two, small)}, short_runs=False,
                   norms=[x / 512.0 for x in (PALETTE * 3)[:n]])
        for r, (k0, k1) in enumerate(runs):
            names = {k: (oov_code(1 + k, 1 + k, 30 + k), self._row("g%d" % k, 1.0)) for k in range(k0, k1)}
            self._pair("all_wild_%d" % r, 1e-2, [], swaps=names)
        self.cap_windows = []
        for p in (self._pair("cap", 1e-2, [], norms=[128.0 + k for k in range(n)]),):
            self.cap_windows.append(p)

    # -- texts
    def _texts(self, stride, seed):
        rng = np.random.default_rng(seed)
        n = self.n
        pal = (112.0, 176.0, 240.0)
        sfill = [self._row("sf%d" % i, p) for i in range(self.n_fill) for p in pal]
        sfill += [self._row("nu%d" % t, 144.0) for t in range(2)]
        sfill += [self._row("u%d" % t, 144.0) for t in range(len(TWINS))]      # (the twins' fan side: a component too)
        ffill = [self._row("ff%d" % i, p) for i in range(self.n_fill) for p in pal]
        ffill += [self._row("nv%d" % t, 144.0) for t in range(2)]
        script = [sfill[i % len(sfill)] for i in range(3)]
        for j, p in enumerate(self.pairs):
            p.s_at = len(script)
            script += p.script
            script += [sfill[int(x)] for x in rng.integers(0, len(sfill), size=3)]
        if self.script_names:
            script[1] = oov_code(20, 44, 61)
        self.script = np.asarray(script, dtype=np.uint32)
        # the fan text: three works; planted windows a stride apart, every eighth one moved to
        # start at 250 .. 256 of a sub-tile of 256 windows; a work ends on one, the stream too
        names = [oov_code(7, 21, 33), oov_code(2, 40, 41), oov_code(11, 11, 50)]
        stream, off = [], [0]

        def fill(count):
            for _ in range(count):
                stream.append(names[int(rng.integers(0, 3))] if rng.random() < 0.02 else
                              ffill[int(rng.integers(0, len(ffill)))])

        cuts = {len(self.pairs) // 3, 2 * len(self.pairs) // 3}
        for j, p in enumerate(self.pairs):
            fill(stride - n - j % 3)
            if j % 8 == 3:
                fill((250 + (j // 8) % 7 - len(stream)) % 256)
            while p.s_at in (len(stream), len(stream) - off[-1]):      # never at its script window's offset
                fill(1)
            p.work, p.f_at, p.stream_at =len(off) - 1, len(stream) - off[-1], len(stream)
            stream += p.fan
            if j + 1 in cuts:
                off.append(len(stream))
        off.append(len(stream))
        self.tok = np.asarray(stream, dtype=np.uint32)
        self.off = np.asarray(off, dtype=np.uint64)

    # -- what the index should find
    def strings(self):
        """(strings, string id per fan token, word per script token)."""
        V = len(self.rows)
        oov = sorted({int(t) for t in self.tok if t & OOV_FLAG})
        strings = ["r%d" % i for i in range(V)] + ["Name%d" % i for i in range(len(oov))]
        sid = {t: V + i for i, t in enumerate(oov)}
        tok_str = np.asarray([sid.get(int(t), int(t)) for t in self.tok], dtype=np.uint32)
        return strings, tok_str, ["sname" if t & OOV_FLAG else "r%d" % int(t) for t in self.script]

    def component_sizes(self):
        """Sizes of the components of `near` over (script row, table row) pairs: the rows of a
        direction the script uses are one component, every other row is alone."""
        used = {self.row_dir[int(t)] for t in self.script if not t & OOV_FLAG}
        sizes, alone = {}, 0
        for r, d in enumerate(self.row_dir):
            if d in used and not str(d).startswith("z"):
                sizes[d] = sizes.get(d, 0) + 1
            else:
                alone += 1
        return sorted(list(sizes.values()) + [1] * alone)

    def fan_component(self, tok, all_wild=False):
        """Component of a fan token under the rule: a class, WILD or NONE (share_comp: without a
        name in the script every fan name is far from everything; with one -- none of its hot
        positions is a fan name's -- those with fewer than three agree with anything)."""
        tok = int(tok)
        if not tok & OOV_FLAG:
            return self.row_dir[tok]
        return WILD if all_wild or (self.script_names and len(oov_hot(tok)) < 3) else NONE

    def q_of(self, tok):
        tok = int(tok)
        return float(len(oov_hot(tok))) if tok & OOV_FLAG else self.q[tok]

    def window(self, fan_toks, all_wild=False):
        """(qi, wild, usable, q) of a fan window, as share_asks sees it."""
        comps = [self.fan_component(t, all_wild) for t in fan_toks]
        q = [self.q_of(t) for t in fan_toks]
        return self.rule.shares(q), [c == WILD for c in comps], [c not in (WILD, NONE) for c in comps], q

    def far_mask(self, pair, all_wild=False):
        m = 0
        for k, (f, s) in enumerate(zip(pair.fan, pair.script)):
            c = self.fan_component(f, all_wild)
            if c != WILD and (c == NONE or c != self.row_dir[int(s)]):
                m |= 1 << k
        return m

    def unconstrained_windows(self, all_wild=False):
        """How many windows of the fan token stream the rule does not constrain."""
        n, count = self.n, 0
        # (where the runs' antichains cannot pass the cap together, the thresholds decide alone)
        short = sum(math.comb(k1 - k0, (k1 - k0) // 2) for k0, k1 in self.runs) <= K_ENUM_CAP
        for p in range(len(self.tok) - n + 1):
            qi, wild, usable, _ = self.window(self.tok[p:p + n], all_wild)
            if short:
                count += any(self.rule.run_threshold(qi, wild, k0, k1) <= 0 for k0, k1 in self.runs)
            else:
                count += self.rule.asks(qi, wild, usable, n) is None
        return count


# ---- which pairs are records, exactly ---------------------------------------------------------

class Exact(object):
    """Dot products of window pairs as integers."""

    def __init__(self, b):
        self.b, self.vec, self.dots = b, {}, {}

    def vector(self, tok):
        tok = int(tok)
        if tok not in self.vec:
            if tok & OOV_FLAG:
                v = [0] * D
                for d in oov_hot(tok):
                    v[d] = 1 << SH
            else:
                v = []
                for x in self.b.emb[tok]:
                    y = float(x) * 2.0 ** SH
                    assert y == int(y)
                    v.append(int(y))
            self.vec[tok] = v
        return self.vec[tok]

    def dot(self, a, b):
        key = (int(a), int(b))
        if key not in self.dots:
            self.dots[key] = sum(x * y for x, y in zip(self.vector(a), self.vector(b)))
        return self.dots[key]

    def is_record(self, pair):
        """cos(F, S) > 1 - thr, thr the double the configuration holds."""
        dot = sum(self.dot(f, s) for f, s in zip(pair.fan, pair.script))
        ff = sum(self.dot(f, f) for f in pair.fan)
        ss = sum(self.dot(s, s) for s in pair.script)
        lim = 1 - Fraction(self.b.thr)
        return dot > 0 and dot * dot * lim.denominator ** 2 > lim.numerator ** 2 * ff * ss

    def cosine(self, a, b):
        return self.dot(a, b) / math.sqrt(self.dot(a, a) * self.dot(b, b))


def family_of(pair):
    name = pair.family
    return name.rsplit("_", 1)[0] if name.rsplit("_", 1)[-1].isdigit() else name
