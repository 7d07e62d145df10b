"""The two oracles across the whole range fs_index_create accepts, not only near the
reference's defaults: NearestFilter(N) for N 1..64, up to 64 tables of few bits and up to
24 bits of few tables, vector widths from 1 to 1024, window sizes 1..16 and thresholds at,
below and around the rounding noise of a window's distance to itself.  CPU only: the
plain-C oracle against the literal Python oracle (canonical mode), plus one known answer
at threshold 0."""

import numpy as np

from hypothesis import HealthCheck, given, settings, strategies as st

from fandom_search_amd import abi
from fandom_search_amd.vocab import oov_vector
from tests import fuzzcase

THRESHOLDS = [-0.1, 0.0, 1e-16, 2.3e-16, 0.02, 0.1, 0.5, 1.0, 2.5]

# (H, B): many tables of few bits, or few tables of many bits (the C oracle and the device
# hold H * (2^B + 1) bucket offsets: B = 24 only with H <= 2)
TABLES = st.one_of(st.tuples(st.integers(1, 64), st.integers(1, 3)),
                   st.tuples(st.integers(1, 2), st.integers(1, 24)))

EDGE_CASE = st.fixed_dictionaries(dict(
    seed=st.integers(0, 2 ** 31 - 1),
    n=st.integers(1, 16),
    HB=TABLES,
    D=st.sampled_from([1, 2, 3, 63, 64, 65, 300, 1024]),
    V=st.integers(3, 12),
    unique=st.booleans(),
    thr=st.sampled_from(THRESHOLDS),
    one_hot=st.booleans(),
    oov_rate=st.sampled_from([0.0, 0.08]),
    n_script=st.integers(0, 60),
    works=st.lists(st.integers(0, 48), min_size=0, max_size=3),
    N=st.one_of(st.integers(1, 64), st.sampled_from([1, 10, 11, 16, 17, 48, 49, 64])),
))


def edge_case(p):
    """fuzzcase.make_case with the drawn (H, B) and NearestFilter size."""
    p = dict(p)
    H, B = p.pop("HB")
    N = p.pop("N")
    if p["one_hot"]:
        p["D"] = max(p["D"], p["V"])
        if p["D"] > 300:                              # (one-hot rows: a narrow table will do)
            p["one_hot"] = False
    case = fuzzcase.make_case(H=H, B=B, **p)
    case["cfg"].nearest_n = N
    return case


def c_oracle_search(case):
    from oracle import c_oracle
    from fandom_search_amd.vocab import pack_strings
    sch, so = pack_strings(case["swords"])
    oi = c_oracle.OracleIndex(case["cfg"], case["script"], sch, so, case["emb"], case["normals"],
                              threads=2)
    return oi.search(case["tok"], case["off"], case["chars"], case["coff"], tok_str=case["tok_str"])


def python_oracle_search(case):
    """Records of the literal restatement (search_restated.AnnIndexSearch, canonical
    arithmetic, NearestFilter(cfg.nearest_n)), work by work."""
    from oracle import nearpy_restated as nr
    from oracle import search_restated as sr
    cfg, emb, strings = case["cfg"], case["emb"], case["strings"]
    D = cfg.emb_dim

    def vec(v):
        return oov_vector(int(v), D) if int(v) & abi.FS_OOV_FLAG else emb[int(v)]

    script_toks = [sr.Tok(w, i, w, i, vec(v)) for i, (w, v) in enumerate(zip(case["swords"], case["script"]))]
    if not script_toks:
        return []
    rows = [[w, 0, 0, "C"] for w in case["swords"]]
    idx = sr.AnnIndexSearch(rows, script_toks, cfg.window_size, cfg.number_of_hashes,
                            cfg.hash_dimensions, cfg.distance_threshold,
                            [case["normals"][h] for h in range(cfg.number_of_hashes)],
                            arith=nr.CanonicalArith(), unique_filter=bool(cfg.unique_filter),
                            nearest=cfg.nearest_n)
    out = []
    off = case["off"]
    for w in range(len(off) - 1):
        lo, hi = int(off[w]), int(off[w + 1])
        fan = [sr.Tok(strings[int(s)], int(s), strings[int(s)].lower(), int(s), vec(v))
               for v, s in zip(case["tok"][lo:hi], case["tok_str"][lo:hi])]
        out += idx.search(w, fan)
    return out


def assert_oracles_agree(case):
    want, _ = c_oracle_search(case)
    py = python_oracle_search(case)
    assert len(py) == len(want)
    for a, b in zip(py, want):
        assert (a[0], a[1], a[4], a[10]) == (b["work"], b["fan_ix"], b["orig_ix"], b["lev"])
        assert np.float64(a[9]).tobytes() == np.float64(b["dist"]).tobytes()
        assert np.float64(a[11]).tobytes() == np.float64(b["comb"]).tobytes()


@settings(max_examples=80, deadline=None, suppress_health_check=list(HealthCheck))
@given(EDGE_CASE)
def test_c_oracle_equals_python_oracle_at_config_edges(p):
    assert_oracles_agree(edge_case(p))


def test_python_oracle_honours_nearest_n():
    """NearestFilter(N) reaches the engine: one script n-gram planted 12 times and one fan
    window equal to it find 12 equal-distance neighbours, of which N are kept in script
    order (a stable sort), so the records' orig_ix move with N."""
    from oracle import nearpy_restated as nr
    from oracle import search_restated as sr
    rng = np.random.default_rng(5)
    D, n = 4, 3
    emb = rng.standard_normal((6, D)).astype(np.float32)
    gram = [1, 2, 3]
    script = []
    for i in range(12):
        script += gram + [4 + i % 2]
    toks = [sr.Tok("w%d" % v, v, "w%d" % v, v, emb[v]) for v in script]
    normals = [rng.standard_normal((2, D * n)) for _ in range(3)]
    for N, want in ((1, 1), (5, 5), (12, 12), (64, 12)):
        idx = sr.AnnIndexSearch([[str(t), 0, 0, "C"] for t in toks], toks, n, 3, 2, 0.1, normals,
                                arith=nr.CanonicalArith(), unique_filter=True, nearest=N)
        hits = idx.engine.neighbours(np.stack([emb[v] for v in gram]).astype(np.float64))
        assert len(hits) <= N
        assert [h[1][0] for h in hits if abs(h[2]) < 1e-12] == [4 * i for i in range(want)]


def canonical_selfdist(emb, script, n):
    """1 - SS / (sqrt(SS) * sqrt(SS)) per script window, in the canonical order: q per
    vector a left-to-right float64 sum of squares, SS a left-to-right sum over the slots."""
    e = emb.astype(np.float64)
    q = np.cumsum(e * e, axis=1)[:, -1]
    out = []
    for s in range(len(script) - n + 1):
        ss = 0.0
        for k in range(n):
            ss = ss + float(q[int(script[s + k])])
        r = np.float64(np.sqrt(ss))
        out.append(float(np.float64(1.0) - np.float64(ss) / (r * r)))
    return np.array(out)


def test_threshold_zero_keeps_the_verbatim_windows_below_zero():
    """Known answer: at threshold 0 a verbatim copy of a script window is kept exactly when
    its canonical distance to itself is below 0 (search.py:184 keeps distance < threshold).
    The table is Gaussian (norms differ), every script n-gram is unique and no other window
    comes within rounding of 0, so the kept (window, script window) pairs are exactly the
    planted ones whose self distance, computed here with numpy, is negative -- and both
    oracles say so."""
    from fandom_search_amd.vocab import pack_strings
    rng = np.random.default_rng(2024)
    n, V, D = 6, 400, 16
    emb = rng.standard_normal((V, D)).astype(np.float32)
    script = rng.permutation(V)[:300].astype(np.uint32)          # distinct ids: unique n-grams
    selfd = canonical_selfdist(emb, script, n)
    assert (selfd < 0).any() and (selfd >= 0).any()
    strings = ["w%d" % i for i in range(V)]
    works, planted = [], []
    for w in range(6):
        fan = rng.integers(0, V, size=120).astype(np.uint32)
        for j in range(4):                                        # spans of n + 3 tokens
            src, dst = int(rng.integers(0, len(script) - n - 3)), 10 + 27 * j
            fan[dst:dst + n + 3] = script[src:src + n + 3]
            planted += [(w, dst + i, src + i) for i in range(4)]
        works.append(fan)
    tok = np.concatenate(works)
    off = np.zeros(len(works) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in works])
    chars, coff = pack_strings(strings)
    case = dict(cfg=abi.make_config(window_size=n, number_of_hashes=4, hash_dimensions=3,
                                    distance_threshold=0.0, emb_dim=D, unique_filter=True),
                emb=emb, normals=rng.standard_normal((4, 3, D * n)), script=script,
                swords=[strings[int(t)] for t in script], tok=tok, tok_str=tok, off=off,
                chars=chars, coff=coff, strings=strings)
    keep = {(w, f, s) for (w, f, s) in planted if selfd[s] < 0}
    rows, st_ = c_oracle_search(case)
    assert st_.matches == len(keep) > 0
    covered = {(w, f + k) for (w, f, s) in keep for k in range(n)}
    assert {(int(r["work"]), int(r["fan_ix"])) for r in rows} == covered
    kept_d = {float(selfd[s]) for (w, f, s) in keep}
    for r in rows:
        assert r["dist"] < 0 and float(r["dist"]) in kept_d
    assert_oracles_agree(case)
