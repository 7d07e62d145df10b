#!/usr/bin/env python3
"""One fan corpus against K scripts: one command against K commands (diagnostic).

  python tools/multi_script_bench.py [--works 20000] [--tokens 2000] [--scripts 4]

Writes a synthetic corpus (synth.write_corpus) and K scripts in the reference's markup into a
temporary directory, then prints one JSON line with
  - the wall time of `ao3.py search corpus s1 .. sK` against the sum of K single-script
    commands, every command in a fresh child process;
  - per 500-work batch, the GPU time (fs_stats.total_ms) of the K searches on one upload (the
    first index's corpus and K - 1 views of it) against K corpora of their own."""

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fandom_search_amd import abi, synth  # noqa: E402


def _command(argv, cwd):
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "ao3.py"), "search"] + argv + ["--synthetic-vocab"],
                       cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode:
        raise SystemExit("ao3.py search failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return time.time() - t0


def _gpu_per_batch(scripts, tokens, reps):
    """Median over `reps` of the summed total_ms of K searches of one 500-work batch."""
    from fandom_search_amd.engine import ScriptIndex
    from fandom_search_amd.vocab import pack_strings
    words = synth.vocab_words()
    emb = synth.embedding()
    normals = synth.lsh_normals(6)
    chars, coff = pack_strings(words)
    cfg = abi.make_config()
    ixs = [ScriptIndex(s, [words[int(t)] for t in s], emb, normals, cfg=cfg) for s in scripts]
    tok, off = synth.corpus_tokens(500, tokens, scripts[0])
    base = ixs[0].corpus(tok, off, chars, coff)
    shared = [base] + [ix.corpus_view(base) for ix in ixs[1:]]
    own = [base] + [ix.corpus(tok, off, chars, coff) for ix in ixs[1:]]
    out = {}
    for name, corpora in (("views", shared), ("own_corpora", own)):
        per = []
        for r in range(reps + 2):
            t = 0.0
            for ix, c in zip(ixs, corpora):
                _, st = ix.search(c, reuse=True)
                assert st.handoff_fallbacks == 0
                t += st.total_ms
            if r >= 2:                                  # (two warm-up rounds)
                per.append(t)
        out[name] = round(float(np.median(per)), 4)
    # what the views save: the K - 1 uploads of the batch (host to device, own corpora only)
    t0 = time.perf_counter()
    for _ in range(reps):
        for c in own[1:]:
            c.update_begin(tok, off)
            c.update_end()
    out["upload_ms_per_own_corpus"] = round(1e3 * (time.perf_counter() - t0) / reps / max(1, len(own) - 1), 4)
    for c in shared[1:] + own[1:] + [base]:
        c.close()
    for ix in ixs:
        ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--works", type=int, default=20000)
    ap.add_argument("--tokens", type=int, default=2000)
    ap.add_argument("--scripts", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    words = synth.vocab_words()
    scripts = [synth.script_tokens(20000, seed=1000 + k) for k in range(a.scripts)]
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        fan = os.path.join(tmp, "fan")
        synth.write_corpus(fan, a.works, a.tokens, scripts[0], words)
        paths = []
        for k, s in enumerate(scripts):
            p = os.path.join(tmp, "script-%d.txt" % k)
            with open(p, "w", encoding="utf8") as fh:
                fh.write(synth.script_markup(s, words))
            paths.append(p)
        t_write = time.time() - t0
        one = _command([fan] + paths + ["--out-dir", os.path.join(tmp, "multi")], tmp)
        singles = [_command([fan, p, "--out-dir", os.path.join(tmp, "single-%d" % k)], tmp)
                   for k, p in enumerate(paths)]
        same = True
        for k in range(a.scripts):
            for i in range((a.works + 499) // 500):
                name = "match-6gram-batch-%d.csv" % i
                with open(os.path.join(tmp, "multi", "script-%d" % k, name), "rb") as f1, \
                        open(os.path.join(tmp, "single-%d" % k, name), "rb") as f2:
                    same = same and f1.read() == f2.read()
    gpu = _gpu_per_batch(scripts, a.tokens, a.reps)
    print(json.dumps({"works": a.works, "tokens_per_work": a.tokens, "scripts": a.scripts,
                      "write_inputs_s": round(t_write, 2),
                      "one_command_s": round(one, 3), "single_commands_s": [round(t, 3) for t in singles],
                      "sum_of_single_commands_s": round(sum(singles), 3),
                      "speedup": round(sum(singles) / one, 2), "batch_files_identical": same,
                      "gpu_ms_per_batch_k_searches": gpu}))


if __name__ == "__main__":
    main()
