#!/usr/bin/env python3
"""Times fs_fanon_dev on synthetic corpora whose tokens are already in device memory.

  python tools/fanon_bench.py [--works 20000] [--tokens 500] [--length 8] [--reps 7]
                              [--check-works 300] [--out profiles/fanon_bench.jsonl]

Four mixes over Zipf tokens of synth's vocabulary:
  plain        nothing planted
  planted      300 phrases of 10 to 40 tokens, each put into 2 to 500 works
  boilerplate  the same 30 tokens at the head of every work
  reposts      1 % of the works are copies of another work
One JSON line per mix: tokens, positions, distinct grams, shared grams, passages and phrases;
the medians over --reps calls (after two warm-up calls) of the per-pass times of fs_fanon_times
and of the call by the host clock, with the spread of the call (min and max); fs_stream_floor
over the same ids beside them (the time one pass over the bytes takes and nothing else); and,
on a corpus of --check-works works of the same mix, the restatement's time and whether the
library's records equal it.  There is no target time.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIXES = ("plain", "planted", "boilerplate", "reposts")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def corpus(mix, n_works, tokens, seed=7):
    """(tok, work_off) of one mix."""
    from fandom_search_amd import synth
    rng = np.random.default_rng(seed)
    tok = synth._draw(rng, n_works * tokens, synth.VOCAB_SIZE).reshape(n_works, tokens)
    if mix == "planted":
        for _ in range(300):
            n = int(rng.integers(10, 41))
            if n > tokens:
                continue
            phrase = synth._draw(rng, n, synth.VOCAB_SIZE)
            into = rng.choice(n_works, size=min(n_works, int(rng.integers(2, 501))), replace=False)
            at = rng.integers(0, tokens - n + 1, size=len(into))
            for w, p in zip(into.tolist(), at.tolist()):
                tok[w, p:p + n] = phrase
    elif mix == "boilerplate":
        n = min(30, tokens)
        tok[:, :n] = synth._draw(rng, n, synth.VOCAB_SIZE)
    elif mix == "reposts":
        copies = rng.choice(n_works, size=max(1, n_works // 100), replace=False)
        for w in copies.tolist():
            tok[w] = tok[(w + 1 + int(rng.integers(0, n_works - 1))) % n_works]
    off = np.arange(n_works + 1, dtype=np.uint64) * np.uint64(tokens)
    return np.ascontiguousarray(tok.reshape(-1)), off


def on_device(a):
    import torch
    return torch.from_numpy(a.view(np.uint8)).to("cuda")


def run(tok, off, length, reps, warmup=2):
    """(records of the last call, totals, per-pass medians, wall times) of fs_fanon_dev."""
    import ctypes as C
    from fandom_search_amd import _lib, abi, engine
    d_tok, d_off = on_device(tok), on_device(off)
    engine.torch_ready()
    L = _lib.load()
    passes, walls, got, totals = [], [], None, {}
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        got = engine.fanon_device(d_tok.data_ptr(), len(tok), d_off.data_ptr(), len(off) - 1,
                                  int(tok.max()) + 1 if len(tok) else 1, length=length,
                                  totals=totals)
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * len(abi.FANON_MS_NAMES))()
        _lib.check(L.fs_fanon_times(ms), "fs_fanon_times")
        if r >= warmup:
            passes.append(list(ms))
            walls.append(wall)
    med = {name: round(median([p[k] for p in passes]), 4)
           for k, name in enumerate(abi.FANON_MS_NAMES)}
    return got, dict(totals), med, walls


def restated(tok, off, length):
    from tests import fanon_restated as fr
    o = [int(x) for x in off]
    works = [tok[o[w]:o[w + 1]].tolist() for w in range(len(o) - 1)]
    t0 = time.perf_counter()
    parts = fr.fanon(works, [], length)
    return parts, time.perf_counter() - t0, fr


def equal(got, parts, fr):
    from fandom_search_amd import abi
    for a, part, keys in zip(got, parts[:4], (fr.WORK_KEYS, fr.GRAM_KEYS, fr.PASSAGE_KEYS,
                                              fr.PHRASE_KEYS)):
        if len(a) != len(part):
            return False
        for name in keys:
            if a[name].tolist() != [d[name] for d in part]:
                return False
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--works", type=int, default=20000)
    ap.add_argument("--tokens", type=int, default=500)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--check-works", type=int, default=300,
                    help="works of the corpus the restatement is run on; 0: none")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fanon_bench.jsonl"))
    args = ap.parse_args()
    from fandom_search_amd import _lib, abi, synth, vocab
    from fandom_search_amd.engine import ScriptIndex
    words = synth.vocab_words()
    script = synth.script_tokens(2000)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(),
                     synth.lsh_normals(6), cfg=abi.make_config(device=0))
    chars, coff = vocab.pack_strings(words)
    lines = []
    for mix in MIXES:
        tok, off = corpus(mix, args.works, args.tokens)
        got, totals, med, walls = run(tok, off, args.length, args.reps)
        c = ix.corpus(tok, off, chars, coff)
        floor = ix.stream_floor(c, reps=20)
        c.close()
        line = {"bench": "fanon", "mix": mix, "source": _lib.source_hash(), "works": args.works,
                "tokens": int(len(tok)), "length": args.length, "positions": totals["positions"],
                "distinct_grams": totals["distinct"], "shared_grams": int(len(got[1])),
                "passages": int(len(got[2])), "phrases": int(len(got[3])), "pass_ms": med,
                "call_ms": round(median(walls), 4), "call_ms_min": round(min(walls), 4),
                "call_ms_max": round(max(walls), 4), "reps": args.reps,
                "stream_floor_ms": round(floor, 4), "id_bytes": int(tok.nbytes)}
        if args.check_works:
            stok, soff = corpus(mix, args.check_works, args.tokens)
            sgot = run(stok, soff, args.length, 1, warmup=0)[0]
            parts, seconds, fr = restated(stok, soff, args.length)
            line.update(check_works=args.check_works, restated_s=round(seconds, 4),
                        equals_restated=equal(sgot, parts, fr))
        lines.append(line)
        print(json.dumps(line), flush=True)
    ix.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
