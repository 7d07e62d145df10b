"""GPU parity at the edges of fs_config: NearestFilter sizes, table counts and widths, vector
widths and window sizes on both sides of every boundary where the pipelines change kernels,
and thresholds at and below the rounding noise of a window's distance to itself.  Every case
is bit-compared with the plain-C oracle, and names the kernel it is there for: a case that
stops reaching its branch fails.

Boundaries (fs_lsh*.hip, fs_api.hip) and the cases on either side of them:
  float32 keys iff C = H * B <= 256          c256 (16 x 16)      | c272 (16 x 17)
    (signs that a wrong decision would flip)   test_gpu_hostile_keys.py: c255_last, c256_last,
                                               c256_col252 | c272_last
  k_lsh_batch / k_lsh_pkeys ballot words     c256, c272          | c336, enum_c336 (16 x 21: a
    (5 words up to C = 320, 6 up to 384)                            sixth word and the zero word)
  wave NearestFilter iff N <= 48             N48                 | N49, N64, serial_N10 (one lane walks)
  k_lsh_lev (lane per match) iff N <= 16     N16                 | N17
  k_lsh_batch iff H <= 16, N <= 48, n in
    {6, 7, 8, 9, 10, 12}                     H16, n7, n12        | H17, n11, n13
  k_lsh_enum iff N <= 10                     enum_N10            | enum_N11
  share rule 2 <= n <= 12, both sides n <= 6 share_n6, share_n7  | share_n13
  exact path, first N occurrences            exact_N1, exact_N10, exact_N64 (70 copies)
  vector widths, window sizes, B             D1 .. D1024, n1 .. n16, B1, B24
  k_cmax tiles of 32 script rows, 256 rows   test_cmax_bounds: 31 / 32 / 33 script rows,
                                             V 255 / 256 / 257, D 1 .. 1024
  k_near_pairs (same tiles)                  test_component_sizes_equal_float64_union_find

Two of these boundaries are branches inside one kernel: float32 against float64 keys, and
the wave against the one-lane NearestFilter.  The launch list cannot tell which side ran
there; bit parity with the oracle on both sides is what covers them.  Cases with no kernel
that must stay absent ("None" below) are those whose other side is such a branch, or whose
boundary is a width, not a kernel choice.
"""

import zlib

import numpy as np
import pytest

from fandom_search_amd import abi, synth
from fandom_search_amd.vocab import pack_strings
from tests import util

pytestmark = pytest.mark.gpu


# ---- inputs ------------------------------------------------------------------

def make_table(kind, V, D, rng):
    if kind == "orth":            # orthogonal rows of different lengths: c_max = 0 (exact path)
        assert V <= D
        emb = np.zeros((V, D), dtype=np.float32)
        emb[np.arange(V), rng.permutation(D)[:V]] = rng.uniform(0.9, 1.1, V).astype(np.float32)
    elif kind == "gauss":         # unrelated rows: a neighbour differs in one slot at most (k_lsh_enum)
        emb = rng.standard_normal((V, D)).astype(np.float32)
    elif kind == "syn":           # the fuzz test's near-synonyms (component prefilters)
        emb = rng.standard_normal((V, D)).astype(np.float32)
        for i in range(1, V, 3):
            emb[i] = emb[i - 1] + 0.15 * rng.standard_normal(D).astype(np.float32)
    elif kind == "real":          # synth.realistic_table (share rule)
        emb, _ = synth.realistic_table(rows=V, dim=D, seed=int(rng.integers(1 << 30)), zero_rows=0)
    elif kind == "dup":           # identical rows under several ids: c_max = 1 (plain LSH)
        emb = rng.standard_normal((V, D)).astype(np.float32)
        emb[V // 2:] = emb[:V - V // 2]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(emb, dtype=np.float32)


def make_case(table="syn", n=6, H=8, B=8, D=16, N=10, thr=0.1, seed=1, V=48, oov=True,
              crowd=70, n_works=6, work_len=360, unique=1, mode=abi.FS_MODE_AUTO):
    """Script and corpus with crowded buckets (one script n-gram `crowd` times, each copy
    with its own strings; identical rows under several ids where the table has them),
    string ids that differ from the vector ids, OOV tokens on both sides (`oov`) and planted
    script spans, verbatim and with one swapped token."""
    rng = np.random.default_rng(seed)
    emb = make_table(table, V, D, rng)
    n_oov = 6

    def oov_id():
        a, b, c = sorted(int(x) for x in rng.integers(0, D, size=3))
        return abi.FS_OOV_FLAG | ((a * D + b) * D + c)

    oovs = [oov_id() for _ in range(n_oov)]
    strings = ["w%d" % i for i in range(V)] + ["W%d" % i for i in range(V)] + \
              ["Oov%d" % i for i in range(n_oov)] + ["w%dx" % i for i in range(V)]
    gram = rng.integers(0, V, size=n).astype(np.uint32)
    script, swords = [], []
    for k in range(crowd):                       # the crowded n-gram, a different spelling each time
        script += [int(t) for t in gram]
        swords += ["w%d" % t + "x" * ((k + j) % 4) for j, t in enumerate(gram)]
        filler = rng.integers(0, V, size=int(rng.integers(1, 4)))
        script += [int(t) for t in filler]
        swords += ["w%d" % t for t in filler]
    rest = rng.integers(0, V, size=500)
    script += [int(t) for t in rest]
    swords += ["w%d" % t for t in rest]
    script = np.asarray(script, dtype=np.uint32)
    if oov:
        for i in rng.choice(len(script), size=4, replace=False):
            k = int(rng.integers(0, n_oov))
            script[i] = oovs[k]
            swords[i] = "oov%d" % k
    works_v, works_s = [], []
    for w in range(n_works):
        v = rng.integers(0, V, size=work_len).astype(np.uint32)
        s = v + np.uint32(V) * rng.integers(0, 2, size=work_len).astype(np.uint32)
        for j in range(6):                       # planted spans, some of them swapped in one slot
            span = int(rng.integers(n, 3 * n + 1))
            src = int(rng.integers(0, len(script) - span))
            dst = int(rng.integers(0, work_len - span))
            v[dst:dst + span] = script[src:src + span]
            s[dst:dst + span] = [2 * V + int(x & 0xFF) % n_oov if x & abi.FS_OOV_FLAG else int(x)
                                 for x in script[src:src + span]]
            if j % 2:
                k = dst + int(rng.integers(0, span))
                if not (v[k] & abi.FS_OOV_FLAG):
                    v[k] = (int(v[k]) ^ 1) % V
                    s[k] = v[k]
        at = int(rng.integers(0, work_len - n))  # the crowded n-gram, spelt as one of its copies
        v[at:at + n] = gram
        s[at:at + n] = gram + np.uint32(2 * V + n_oov) * np.uint32(w % 2)
        if oov:
            for i in rng.choice(work_len, size=8, replace=False):
                k = int(rng.integers(0, n_oov))
                v[i] = oovs[k]
                s[i] = 2 * V + k
        works_v.append(v)
        works_s.append(s)
    off = np.zeros(n_works + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in works_v])
    chars, coff = pack_strings(strings)
    cfg = abi.make_config(window_size=n, number_of_hashes=H, hash_dimensions=B, distance_threshold=thr,
                          emb_dim=D, nearest_n=N, unique_filter=unique, mode=mode)
    return dict(cfg=cfg, emb=emb, normals=rng.standard_normal((H, B, D * n)), script=script, swords=swords,
                tok=np.concatenate(works_v), tok_str=np.concatenate(works_s), off=off, chars=chars, coff=coff)


def oracle_rows(case):
    from oracle import c_oracle
    sch, so = pack_strings(case["swords"])
    oi = c_oracle.OracleIndex(case["cfg"], case["script"], sch, so, case["emb"], case["normals"], threads=8)
    return oi.search(case["tok"], case["off"], case["chars"], case["coff"], tok_str=case["tok_str"])


def launches(ix, corpus, n_rows):
    """Kernel names of one profiled search of `corpus` (fs_search_profile)."""
    import torch
    cap = n_rows + 1024
    buf = torch.zeros(32 * cap + 64, dtype=torch.uint8, device="cuda")
    names = [k for k, _ in ix.profile(corpus, buf.data_ptr() + 32, cap)]
    torch.cuda.synchronize()
    return names


def run_case(case):
    """HIP rows against the oracle's; returns (index, corpus, rows, stats)."""
    from fandom_search_amd.engine import ScriptIndex
    want, ost = oracle_rows(case)
    ix = ScriptIndex(case["script"], case["swords"], case["emb"], case["normals"], cfg=case["cfg"])
    c = ix.corpus(case["tok"], case["off"], case["chars"], case["coff"], tok_str=case["tok_str"])
    got, st = ix.search(c)
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches and st.windows_processed == ost.windows_processed
    return ix, c, got, st


# ---- the table of cases --------------------------------------------------------

GEN, EXACT = abi.FS_MODE_GENERAL, abi.FS_MODE_EXACT
LEV_LANE = {"FS_LSH_LEV_LANE": "2"}        # the deferred Levenshtein forms whatever the last search found

# name: (make_case arguments, environment, kernel that must be launched, kernel that must not be, path)
CASES = {
    # NearestFilter size
    "N1": (dict(N=1), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "N2": (dict(N=2), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "N10": (dict(N=10), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "N11": (dict(N=11), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "N16": (dict(N=16), LEV_LANE, "k_lsh_lev", "k_lsh_verify", GEN),
    "N17": (dict(N=17), LEV_LANE, "k_lsh_verify", "k_lsh_lev", GEN),
    "N48": (dict(N=48), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "N49": (dict(N=49), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "N64": (dict(N=64, unique=0), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "serial_N10": (dict(N=10), dict(LEV_LANE, FS_LSH_SERIAL="1"), "k_lsh_verify", "k_lsh_batch", GEN),
    "enum_N10": (dict(table="gauss", D=64, N=10, oov=False), LEV_LANE, "k_lsh_enum", None, GEN),
    "enum_N11": (dict(table="gauss", D=64, N=11, oov=False), LEV_LANE, "k_lsh_batch", "k_lsh_enum", GEN),
    # tables
    "H1": (dict(H=1, B=12), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "H16": (dict(H=16, B=4), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "H17": (dict(H=17, B=4), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "H64": (dict(H=64, B=2, unique=0), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "c256": (dict(H=16, B=16), LEV_LANE, "k_lsh_batch", None, GEN),
    "c272": (dict(H=16, B=17), LEV_LANE, "k_lsh_batch", None, GEN),
    "c336": (dict(H=16, B=21), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "enum_c336": (dict(table="gauss", D=64, H=16, B=21, oov=False), LEV_LANE, "k_lsh_enum", None, GEN),
    "B1": (dict(H=16, B=1), LEV_LANE, "k_lsh_batch", None, GEN),
    "B24": (dict(H=2, B=24), LEV_LANE, "k_lsh_batch", None, GEN),
    # vector widths
    "D1": (dict(table="dup", D=1, V=8), {}, "k_lsh_scan", None, GEN),
    "D3": (dict(table="syn", D=3, V=12), LEV_LANE, "k_lsh_scan", None, GEN),
    "D64": (dict(table="orth", D=64, V=48, oov=False), {}, "k_scan", "k_lsh", EXACT),
    "D65": (dict(table="syn", D=65), LEV_LANE, "k_share_scan", None, GEN),
    "D300": (dict(table="syn", D=300), LEV_LANE, "k_share_scan", None, GEN),
    "D1024": (dict(table="syn", D=1024, V=24, work_len=200), LEV_LANE, "k_share_scan", None, GEN),
    # window sizes
    "n1": (dict(n=1, V=24), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "n2": (dict(n=2), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "n7": (dict(n=7), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "n11": (dict(n=11), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "n12": (dict(n=12), LEV_LANE, "k_lsh_batch", "k_lsh_verify", GEN),
    "n13": (dict(n=13), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    "n16": (dict(n=16), LEV_LANE, "k_lsh_verify", "k_lsh_batch", GEN),
    # the table kinds the pipelines pick
    "share_n6": (dict(table="real", D=64, V=400, oov=False), {}, "k_share_scan<6>", None, GEN),
    "share_n7": (dict(table="real", D=64, V=400, n=7, oov=False), {}, "k_share_scan<7>", None, GEN),
    "share_n13": (dict(table="real", D=64, V=400, n=13, oov=False), {}, "k_lsh_scan", "k_share", GEN),
    "plain_dup": (dict(table="dup", D=16), {}, "k_lsh_scan", None, GEN),
    # the exact path: the first N occurrences of a crowded n-gram (70 copies)
    "exact_N1": (dict(table="orth", D=64, N=1, oov=False), {}, "k_scan", "k_lsh", EXACT),
    "exact_N10": (dict(table="orth", D=64, N=10, oov=False), {}, "k_scan", "k_lsh", EXACT),
    "exact_N64": (dict(table="orth", D=64, N=64, oov=False, unique=0), {}, "k_scan", "k_lsh", EXACT),
    "exact_n1_N11": (dict(table="orth", D=64, n=1, N=11, oov=False), {}, "k_scan", "k_lsh", EXACT),
    "exact_n16_N17": (dict(table="orth", D=64, n=16, N=17, thr=0.02, oov=False), {}, "k_scan", "k_lsh", EXACT),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_config_edge_equals_oracle(name, monkeypatch):
    kw, env, kernel, absent, path = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)             # switches are read when the index is built
    ix, c, got, st = run_case(make_case(seed=zlib.crc32(name.encode()) & 0xFFFF, **kw))
    assert ix.info["path"] == path and st.path == path
    assert len(got) > 0
    names = launches(ix, c, len(got))
    assert any(k.startswith(kernel) for k in names), (kernel, names)
    assert absent is None or not any(k.startswith(absent) for k in names), (absent, names)
    ix.close()


# ---- thresholds at and below the noise -------------------------------------------

NOISE_THRESHOLDS = [-1e-3, 0.0, 1e-16, 2.3e-16, 1e-15, 1.0, 2.5]


@pytest.mark.parametrize("mode", [abi.FS_MODE_AUTO, abi.FS_MODE_GENERAL, abi.FS_MODE_EXACT])
@pytest.mark.parametrize("n", [6, 4])
@pytest.mark.parametrize("thr", NOISE_THRESHOLDS)
def test_thresholds_at_the_noise(n, thr, mode):
    """Orthogonal rows of different lengths (c_max = 0: the cosine bound of the exact proof
    holds for any small threshold) and verbatim spans: a window's distance to itself is
    rounding noise around 0, so at thresholds of that size the reference keeps
    some verbatim windows and drops others (search.py:184).  AUTO and GENERAL equal the
    oracle, AUTO on the LSH pipeline below and within the noise and on the exact path above
    it; EXACT equals the oracle above the noise and refuses with FS_E_UNPROVEN, naming the
    reason, below it and where the cosine bound fails (thresholds 1 and 2.5)."""
    from fandom_search_amd import _lib
    case = make_case(table="orth", D=64, n=n, thr=thr, oov=False, seed=7, mode=mode, N=10)
    in_noise = not (2e-16 < thr < 1e-3)
    if mode == abi.FS_MODE_EXACT and (in_noise or thr >= 1.0):
        with pytest.raises(_lib.FsError) as e:
            run_case(case)
        assert e.value.code == abi.FS_E_UNPROVEN
        assert ("cos bound" if thr >= 1.0 else "distance to itself") in str(e.value)
        return
    ix, _, got, _ = run_case(case)
    assert len(got) > 0 or thr < 0
    assert ix.info["path"] == (GEN if mode == abi.FS_MODE_GENERAL or in_noise else EXACT)
    ix.close()


# ---- the float32 build-time bound c_max at its lines ----------------------------------

def canonical_q(emb):
    e = emb.astype(np.float64)
    return np.cumsum(e * e, axis=1)[:, -1]


def true_cmax(emb, rows):
    """Largest cosine (float64) between a script row and any other table row, 0 at least."""
    e = emb.astype(np.float64)
    u = e / np.linalg.norm(e, axis=1, keepdims=True)
    cos = u[rows] @ u.T
    cos[np.arange(len(rows)), rows] = -2.0
    return max(0.0, float(cos.max()))


def line_threshold(c_line, q):
    """The threshold at which the proof's bound for n = 2 equals 1 - threshold at c = c_line."""
    qmin, qmax = float(q.min()), float(q.max())
    return 1.0 - (qmax + c_line * qmin) / (qmax + qmin)


def first_appearance(script):
    """The script's distinct rows in order of first appearance: rows_u of prove_exact and of
    the component builds, which k_cmax / k_near_pairs stage 32 at a time."""
    _, first = np.unique(script, return_index=True)
    return script[np.sort(first)]


def tail_table(rng, V, D, R, partner_cos=0.97):
    """Unit rows scaled by U(0.95, 1.05) (norms within 10 % of each other) and a script of R
    distinct rows whose last row in first-appearance order (rows_u[R - 1]: the 33rd, alone in
    the second tile of script rows, at R = 33) is partnered at cosine `partner_cos` with table
    row V - 1 (row 256, alone in the second block of table rows, at V = 257), outside the script."""
    emb = rng.standard_normal((V, D))
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    emb *= rng.uniform(0.95, 1.05, (V, 1))
    rows = rng.choice(V - 1, size=R, replace=False)
    last = int(rows[-1])
    if D > 1:
        u = emb[last] / np.linalg.norm(emb[last])
        w = rng.standard_normal(D)
        w -= (w @ u) * u
        emb[V - 1] = np.linalg.norm(emb[V - 1]) * (partner_cos * u + np.sqrt(1 - partner_cos ** 2) * w / np.linalg.norm(w))
    script = np.concatenate([rng.permutation(np.repeat(rows[:-1], 3)), [last] * 3]).astype(np.uint32)
    rows_u = first_appearance(script)
    assert len(rows_u) == R and rows_u[-1] == last and last != V - 1
    return emb.astype(np.float32), script, last


def unit_cos(emb):
    e = emb.astype(np.float64)
    u = e / np.linalg.norm(e, axis=1, keepdims=True)
    return u @ u.T


@pytest.mark.parametrize("R,V", [(31, 255), (32, 256), (33, 257)])
@pytest.mark.parametrize("D", [1, 64, 65, 300, 1024])
def test_cmax_bounds(D, R, V):
    """k_cmax stages 32 script rows per block (32 * D floats of LDS, 128 KiB at D = 1024) and
    takes 256 table rows per block.  The decisive pair sits in both tails: the last script row
    in first-appearance order against table row V - 1 (tail_table), every other pair at least
    1e-3 below it, so a tile that drops either tail moves c_max by more than the 1e-4 the test
    allows (D = 1: every cosine is +-1, only soundness and the decision are tested).  c_max is
    sound and within 1e-4 of the float64 value, and proof_ok equals the float64 decision when
    the true c is 2e-4 from the line, on either side.  (Norms within 10 % of each other, so
    a_min^2 / (a_max^2 + a_min^2) > 0.4: 2e-4 from the line in c is 8e-5 in the bound, far
    beyond the proof's 1e-4 slack on c_max plus its 1e-6 margin on the bound.)"""
    from fandom_search_amd.engine import ScriptIndex
    rng = np.random.default_rng(D * 1000 + R)
    emb, script, last = tail_table(rng, V, D, R)
    rows = first_appearance(script)
    true = true_cmax(emb, rows)
    if D > 1:
        cos = unit_cos(emb)[rows]
        cos[np.arange(R), rows] = -2.0
        top = cos.max()                                  # the pair in both tails decides
        assert np.unravel_index(np.argmax(cos), cos.shape) == (R - 1, V - 1)
        cos[R - 1, V - 1] = -2.0
        assert cos.max() < top - 1e-3
    q = canonical_q(emb)
    swords = ["w%d" % t for t in script]
    for above in ((True, False) if true < 0.999 else (True,)):     # true c above / below the line
        thr = line_threshold(true - 2e-4 if above else true + 2e-4, q)
        cfg = abi.make_config(window_size=2, number_of_hashes=1, hash_dimensions=4, emb_dim=D,
                              distance_threshold=thr)
        ix = ScriptIndex(script, swords, emb, rng.standard_normal((1, 4, 2 * D)), cfg=cfg)
        cmax = ix.info["c_max"]
        assert cmax + 1e-4 >= true and abs(cmax - true) <= 1e-4, (cmax, true)
        assert ix.info["proof_ok"] == (0 if above else 1), (above, cmax, true, thr)
        ix.close()


def union_find_sizes(V, pairs):
    """Component sizes, components in order of their smallest member (fs_build_components)."""
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    sizes, id_of = [], {}
    for v in range(V):
        r = find(v)
        if r not in id_of:
            id_of[r] = len(sizes)
            sizes.append(0)
        sizes[id_of[r]] += 1
    return sizes


@pytest.mark.parametrize("rule", ["components", "share"])
@pytest.mark.parametrize("R,V", [(31, 255), (33, 257)])
def test_component_sizes_equal_float64_union_find(rule, R, V, monkeypatch):
    """k_near_pairs (k_cmax's tiling) gives the pairs behind the component ids: near iff
    cos(u, v) > 1 - T / (2 |u| |v|), T = n * thr * a_max^2, for the component prefilters
    (DESIGN 4), or cos(u, v) > gamma for the share rule (FS_LSH_SYN=0 builds it
    instead).  With every (script row, table row) pair at least 2e-4 from its line,
    component_sizes() equals a float64 union-find's.  Planted near pairs, one of them in both
    tails (tail_table) and a component of three, make the components differ from singletons."""
    from fandom_search_amd.engine import ScriptIndex
    if rule == "share":
        monkeypatch.setenv("FS_LSH_SYN", "0")
    rng = np.random.default_rng(R * 7 + V)
    n, D, thr = 6, 300, 0.1
    emb, script, last = tail_table(rng, V, D, R, partner_cos=0.95)
    rows = first_appearance(script)
    e = emb.astype(np.float64)
    nrm = np.linalg.norm(e, axis=1)
    outside = np.setdiff1d(np.arange(V - 1), rows)
    for i in range(4):                               # more near pairs: script row -> table row outside
        a, b = int(rows[3 * i]), int(outside[i])
        w = rng.standard_normal(D)
        w -= (w @ e[a]) / (e[a] @ e[a]) * e[a]
        e[b] = nrm[b] * (0.95 * e[a] / nrm[a] + np.sqrt(1 - 0.95 ** 2) * w / np.linalg.norm(w))
    a, c = int(rows[0]), int(rows[2])                # a script row near rows[0] and its partner: three
    w = rng.standard_normal(D)
    w -= (w @ e[a]) / (e[a] @ e[a]) * e[a]
    e[c] = nrm[c] * (0.96 * e[a] / nrm[a] + np.sqrt(1 - 0.96 ** 2) * w / np.linalg.norm(w))
    emb = e.astype(np.float32)
    cos = unit_cos(emb)[rows]
    q = canonical_q(emb)
    if rule == "share":
        line = np.full(cos.shape, 0.7)                # the share rule's default gamma
    else:
        norms = np.sqrt(q)
        line = 1.0 - n * thr * float(q.max()) / (2.0 * np.outer(norms[rows], norms))
    far_from_line = np.abs(cos - line)
    far_from_line[np.arange(len(rows)), rows] = 1.0
    assert far_from_line.min() >= 2e-4
    near = cos > line
    near[np.arange(len(rows)), rows] = False
    want = union_find_sizes(V, [(int(rows[i]), int(v)) for i, v in zip(*np.nonzero(near))])
    assert max(want) >= 3 and near[R - 1, V - 1]
    cfg = abi.make_config(window_size=n, emb_dim=D, distance_threshold=thr)
    ix = ScriptIndex(script, ["w%d" % t for t in script], emb, rng.standard_normal((15, 14, n * D)), cfg=cfg)
    assert ix.info["proof_ok"] == 0
    if rule == "share":
        assert ix.share_info()["gamma"] == 0.7 and ix.share_info()["components"] == len(want)
    sizes, _ = ix.component_sizes()
    assert [int(x) for x in sizes] == want
    ix.close()


def test_proof_fails_just_above_the_line():
    """c 1e-5 above the line: the proof must fail, and a fan window that swaps the script's
    short vector u for its partner v (cosine c) -- the pair the bound is tight for, next to
    the longest vector -- lies within the threshold and is found, as by the oracle."""
    rng = np.random.default_rng(17)
    V, D = 64, 64
    emb = rng.standard_normal((V, D))
    emb = 2.0 * emb / np.linalg.norm(emb, axis=1, keepdims=True)
    u = emb[0] / 2.0
    w = rng.standard_normal(D)
    w -= (w @ u) * u
    c = 0.9
    emb[0], emb[1] = u, c * u + np.sqrt(1 - c * c) * w / np.linalg.norm(w)
    emb = emb.astype(np.float32)
    q = canonical_q(emb)
    b = int(np.argmax(q))
    true = true_cmax(emb, np.array([0, b] + list(range(2, 40))))
    thr = line_threshold(true - 1e-5, q)
    script = np.concatenate([rng.integers(2, 40, size=300), [b, 0], rng.integers(2, 40, size=300)])
    swords = ["w%d" % t for t in script]
    tok = rng.integers(2, 40, size=400)
    tok[100:102] = [b, 1]
    tok[250:252] = [b, 0]
    strings = ["w%d" % i for i in range(V)]
    chars, coff = pack_strings(strings)
    cfg = abi.make_config(window_size=2, number_of_hashes=15, hash_dimensions=4, emb_dim=D,
                          distance_threshold=thr)
    case = dict(cfg=cfg, emb=emb, normals=rng.standard_normal((15, 4, 2 * D)), script=script.astype(np.uint32),
                swords=swords, tok=tok.astype(np.uint32), tok_str=tok.astype(np.uint32),
                off=np.array([0, 400], dtype=np.uint64), chars=chars, coff=coff)
    ix, _, got, st = run_case(case)
    assert ix.info["proof_ok"] == 0 and st.path == GEN
    assert abs(ix.info["c_max"] - true) <= 1e-4
    swap = got[(got["fan_ix"] == 101) & (got["orig_ix"] == 301)]
    assert len(swap) == 1 and 0 < swap["dist"][0] < thr
    ix.close()


# ---- one step past each limit ---------------------------------------------------

@pytest.mark.parametrize("field,value", [("window_size", 0), ("window_size", 17), ("number_of_hashes", 0),
                                         ("number_of_hashes", 65), ("hash_dimensions", 0),
                                         ("hash_dimensions", 25), ("emb_dim", 0), ("emb_dim", 1025),
                                         ("nearest_n", 0), ("nearest_n", 65)])
def test_limits_are_refused(field, value):
    from fandom_search_amd import _lib
    from fandom_search_amd.engine import ScriptIndex
    kw = dict(window_size=2, number_of_hashes=1, hash_dimensions=1, emb_dim=4, nearest_n=10)
    kw[field] = value
    cfg = abi.make_config(**kw)
    emb = np.ones((3, kw["emb_dim"]), dtype=np.float32)
    normals = np.zeros(kw["number_of_hashes"] * kw["hash_dimensions"] * kw["emb_dim"] * kw["window_size"])
    with pytest.raises(_lib.FsError) as e:
        ScriptIndex(np.array([0, 1, 2], dtype=np.uint32), ["a", "b", "c"], emb, normals, cfg=cfg)
    assert e.value.code == abi.FS_E_UNSUPPORTED
