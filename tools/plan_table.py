#!/usr/bin/env python3
"""What a search launches, case by case (diagnostic; tests/test_gpu_plan_table.py).

  python tools/plan_table.py [--case NAME] > plan_table.json

For a fixed list of cases -- an index recipe plus FS_* switches -- builds the index and a
corpus and prints one JSON object per case: the kernel name and the scan shape asked before
the search, the index's path, and after one search the path it took, its scan launches, its
hand-off fallbacks and its number of rows.  Only the public Python API is asked, so the
same file runs on any commit: tests/golden/plan_table.json is the output of the commit
before the planner (fs_plan.hip), and the test holds every later tree to it.

Without --case every case runs in a process of its own, with its switches in the
environment from the start (a switch read once per process is then seen as well as one read
per index).  run_case() runs one case in this process."""
import functools
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from fandom_search_amd import abi, synth
from fandom_search_amd.vocab import pack_strings

SCRIPT_TOKENS = 4000


def _lengths(n):
    """A handful of works of 300 to 600 tokens, an empty one and one of n - 1 tokens."""
    return [300, 450, 600, 512, 0, n - 1, 380, 555]


def _ragged(lengths, script, vocab_size=synth.VOCAB_SIZE):
    parts = [synth.fanwork_tokens(i, int(k), script, vocab_size) if k else np.zeros(0, np.uint32)
             for i, k in enumerate(lengths)]
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.concatenate(parts).astype(np.uint32), off


@functools.lru_cache(maxsize=None)
def _base():
    words = synth.vocab_words()
    chars, coff = pack_strings(words)
    return words, synth.embedding(), chars, coff


@functools.lru_cache(maxsize=None)
def _recipe(kind, n):
    """-> dict(cfg, script, swords, emb, normals, tok, off, chars, coff, tok_str)"""
    words, emb, chars, coff = _base()
    r = {"tok_str": None, "normals": synth.lsh_normals(n), "cfg": abi.make_config(window_size=n)}
    if kind in ("exact", "exact_str", "exact_oov", "general"):
        # the synthetic table: the exact n-gram proof holds up to n = 6 and fails by one slot at n = 8
        script = synth.script_tokens(SCRIPT_TOKENS)
        tok, off = _ragged(_lengths(n), script)
        r.update(script=script, swords=[words[int(t)] for t in script], emb=emb, tok=tok, off=off,
                 chars=chars, coff=coff)
        if kind == "exact_str":
            # string ids of the batch's own: lower-case, Capitalised, UPPER + '!!'
            strings = list(words) + [w.capitalize() for w in words] + [w.upper() + "!!" for w in words]
            variant = np.random.default_rng(5).choice(3, size=len(tok), p=[0.34, 0.33, 0.33]).astype(np.uint32)
            r["tok_str"] = (tok + variant * len(words)).astype(np.uint32)
            r["chars"], r["coff"] = pack_strings(strings)
        if kind == "exact_oov":
            tok = tok.copy()
            tok[5::97] = abi.FS_OOV_FLAG | ((1 * 300 + 2) * 300 + 3)
            r["tok"] = tok
            r["tok_str"] = np.where(tok & abi.FS_OOV_FLAG, len(words), tok).astype(np.uint32)
            r["chars"], r["coff"] = pack_strings(list(words) + ["Zzz"])
    elif kind == "one_hot":
        # 256 one-hot vectors: c_max = 0, the proof holds at every window size below the threshold
        V = 256
        w1 = synth.vocab_words(V)
        script = synth.script_tokens(SCRIPT_TOKENS, vocab_size=V)
        tok, off = _ragged(_lengths(n), script, V)
        r["chars"], r["coff"] = pack_strings(w1)
        r["cfg"] = abi.make_config(window_size=n, distance_threshold=0.05)
        r.update(script=script, swords=[w1[int(t)] for t in script],
                 emb=np.eye(V, synth.EMB_DIM, dtype=np.float32), tok=tok, off=off)
    elif kind == "synonyms":
        # groups of eight near-synonyms: the prefilters over component ids
        emb_c, perm = synth.clustered_table()
        script = synth.script_tokens(SCRIPT_TOKENS)
        tok, off = _ragged(_lengths(n), script)
        r.update(script=script, swords=[words[int(t)] for t in script], emb=emb_c,
                 tok=synth.synonym_swaps(tok, perm), off=off, chars=chars, coff=coff)
    elif kind == "realistic":
        # unnormalised vectors in nested groups: no integer prefilter applies, the share rule does
        rows = 6000
        emb_r, group = synth.realistic_table(rows=rows)
        strings, vid = synth.realistic_vector_ids(rows)
        script = synth._draw(np.random.default_rng(77), SCRIPT_TOKENS, rows)
        tok_str, _ = synth.realistic_corpus(8, 500, script, group, rows, oov_rate=0.0)
        for j in range(4):
            tok_str[50 + 900 * j:64 + 900 * j] = script[200 + 40 * j:214 + 40 * j]
        lengths = [500, 300, 600, 400, 450, 0, n - 1, 550, 595, 600]
        off = np.zeros(len(lengths) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lengths)
        assert int(off[-1]) == len(tok_str)
        r["chars"], r["coff"] = pack_strings(strings)
        r.update(script=script, emb=emb_r, tok=vid[tok_str], off=off, tok_str=tok_str.astype(np.uint32),
                 swords=[strings[int(t)].upper() if i % 9 == 0 else strings[int(t)] for i, t in enumerate(script)])
    else:
        raise ValueError(kind)
    return r


# name -> (recipe, n, switches, view)
CASES = {}


def _add(name, kind, n, env=None, view=None):
    CASES[name] = (kind, n, dict(env or {}), view)


for _name, _env in (("default", {}), ("scan_rows_0", {"FS_SCAN_ROWS": "0"}), ("scan_tpl_4", {"FS_SCAN_TPL": "4"}),
                    ("scan_variant_simple", {"FS_SCAN_VARIANT": "simple"}), ("scan_direct_0", {"FS_SCAN_DIRECT": "0"}),
                    ("scan_capw_2", {"FS_SCAN_CAPW": "2"}), ("ranges_caprow_2", {"FS_RANGES_CAPROW": "2"}),
                    ("lanes_4", {"FS_LANES": "4"}), ("rows_waves_4", {"FS_ROWS_WAVES": "4"}),
                    ("wait_spins_0", {"FS_WAIT_SPINS": "0"}), ("host_wire8_0", {"FS_HOST_WIRE8": "0"})):
    _add("exact4_" + _name, "exact", 4, _env)
_add("exact4_str_fused_0", "exact_str", 4, {"FS_STR_FUSED": "0"})
_add("exact9_one_hot", "one_hot", 9)
_add("exact12_one_hot", "one_hot", 12)
_add("exact6_oov_batch", "exact_oov", 6)
for _name, _env in (("default", {}), ("near_fused_0", {"FS_NEAR_FUSED": "0"}), ("scan_near8_0", {"FS_SCAN_NEAR8": "0"}),
                    ("lsh_prefilter_0", {"FS_LSH_PREFILTER": "0"}), ("scan_capw_2", {"FS_SCAN_CAPW": "2"})):
    _add("general8_" + _name, "general", 8, _env)
_add("synonyms6_default", "synonyms", 6)
_add("synonyms6_near_fused_0", "synonyms", 6, {"FS_NEAR_FUSED": "0"})
_add("realistic6_default", "realistic", 6)
_add("realistic6_lsh_share_0", "realistic", 6, {"FS_LSH_SHARE": "0"})
_add("view_of_another_index", "exact", 4, view="live")
_add("view_detached", "exact", 4, view="detached")


def run_case(name):
    """One case in this process -> the dict that is printed (and compared)."""
    from fandom_search_amd.engine import ScriptIndex
    kind, n, env, view = CASES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    out = {"case": name}
    try:
        r = _recipe(kind, n)
        ix = ScriptIndex(r["script"], r["swords"], r["emb"], r["normals"], cfg=r["cfg"])
        c = base = other = None
        if view:
            # a second index over the other half of the script order; the view searches its corpus
            rev = r["script"][::-1].copy()
            other = ScriptIndex(rev, r["swords"][::-1], r["emb"], r["normals"], cfg=r["cfg"])
            base = other.corpus(r["tok"], r["off"], r["chars"], r["coff"], tok_str=r["tok_str"])
            c = ix.corpus_view(base)
            if view == "detached":
                base.close()
                base = None
        else:
            c = ix.corpus(r["tok"], r["off"], r["chars"], r["coff"], tok_str=r["tok_str"])
        out["kernel_name"] = ix.kernel_name(c)
        out["info_path"] = int(ix.info["path"])
        if view == "detached":
            # every call on it but its destruction is refused
            out["scan_shape"] = out["st_path"] = out["scan_launches"] = out["handoff_fallbacks"] = out["rows"] = None
        else:
            out["scan_shape"] = ix.scan_shape(c)
            rows, st = ix.search(c)
            out["st_path"] = int(st.path)
            out["scan_launches"] = int(st.scan_launches)
            out["handoff_fallbacks"] = int(st.handoff_fallbacks)
            out["rows"] = int(len(rows))
        c.close()
        if base is not None:
            base.close()
        if other is not None:
            other.close()
        ix.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def main(argv):
    if len(argv) == 2 and argv[0] == "--case":
        t0 = time.perf_counter()
        print(json.dumps(run_case(argv[1]), sort_keys=True))
        sys.stderr.write("%-28s %.2f s\n" % (argv[1], time.perf_counter() - t0))
        return 0
    for name in CASES:
        env = dict(os.environ)
        env.update(CASES[name][2])
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--case", name], env=env, timeout=180)
        if rc != 0:
            sys.stderr.write("case %s failed (exit status %d)\n" % (name, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
