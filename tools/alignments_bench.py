#!/usr/bin/env python3
"""`alignments` timings, one JSON line per shape of the records:
  records        N synthetic match records sorted by (work, fan_ix): the three mixes of
                 tools/works_bench.py (small, medium, large); `noisy`: the medium mix with one
                 record in ten turned into a stray and one link in ten given an inserted or a
                 dropped word; `transcript`: one work of N records in one segment, the chain
                 pass's slow case (one wave, N dependent steps)
  alignments_ms  fs_alignments_rows on those records already in HBM (median of --reps calls
                 after a warm-up, host clock around the synchronous call)
  pass_ms        its passes by HIP events (fs_alignments_times), the median of each over the
                 same calls
  passages_ms    fs_passages_rows on the same records in the same process, the same way: the
                 floor the call cannot go under (it reads the same records once); ratio =
                 alignments_ms / passages_ms
  alignments, path_records, longest, segments_over_8   what was found (the defaults: --min-words
                 6, --reach 4, --match 2, --gap 1)
  checked        the first --oracle-records records, through fs_alignments, were compared with
                 the test oracle (tests/alignments_restated.py), every field and the path list

usage: python tools/alignments_bench.py [--records N] [--reps R]
                                        [--shapes small,medium,large,noisy,transcript]
                                        [--oracle-records K] [--device D]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tools"))

from works_bench import N_SCRIPT, records   # noqa: E402

M, R, S, P = 6, 4, 2, 1


def noisy(n, seed=2):
    work, fan, orig, dist, comb = records(n, "medium")
    rng = np.random.default_rng(seed)
    kind = rng.random(n)
    fan = fan.astype(np.int64) + np.cumsum(kind < 0.05)            # an inserted word
    orig = orig.astype(np.int64) + np.cumsum((kind >= 0.05) & (kind < 0.1))   # a dropped word
    stray = rng.random(n) < 0.1
    orig = np.where(stray, rng.integers(0, N_SCRIPT, size=n), orig % N_SCRIPT)
    return (work, fan.astype(np.uint32), orig.astype(np.uint32), dist, comb)


def transcript(n, seed=3):
    rng = np.random.default_rng(seed)
    kind = rng.random(n)
    fan = np.cumsum(1 + (kind < 0.05))
    orig = np.cumsum(1 + ((kind >= 0.05) & (kind < 0.1)))
    dist = rng.random(n) * 0.1
    return (np.zeros(n, dtype=np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), dist,
            dist * rng.integers(0, 8, size=n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,noisy,transcript")
    ap.add_argument("--oracle-records", type=int, default=200_000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    n = args.records

    import torch
    from fandom_search_amd import _lib, abi, alignments, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    L = _lib.load()
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    dev = "cuda:%d" % args.device
    for shape in args.shapes.split(","):
        cols = noisy(n) if shape == "noisy" else transcript(n) if shape == "transcript" \
            else records(n, shape)
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix", "dist", "comb"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        cap = n // M + 1
        d_out = torch.empty(cap * abi.ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_path = torch.empty(n, dtype=torch.int32, device=dev)
        d_pass = torch.empty(cap * abi.PASSAGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        host, passes, found = [], [], (0, 0)
        ms = (C.c_double * 6)()
        for rep in range(args.reps + 1):                    # the first call is the warm-up
            t = time.perf_counter()
            found = ix.alignments_device(d_rows.data_ptr(), n, M, R, S, P,
                                         out_ptrs=(d_out.data_ptr(), d_path.data_ptr()),
                                         caps=(cap, n))
            host.append((time.perf_counter() - t) * 1e3)
            L.fs_alignments_times(ms)
            passes.append(list(ms))
        floor = []
        for rep in range(args.reps + 1):
            t = time.perf_counter()
            ix.passages_device(d_rows.data_ptr(), n, M, 0, out_ptr=d_pass.data_ptr(), cap=cap)
            floor.append((time.perf_counter() - t) * 1e3)
        got = d_out[:found[0] * abi.ALIGNMENT_DTYPE.itemsize].cpu().numpy().view(abi.ALIGNMENT_DTYPE)
        fan = cols[1].astype(np.int64)
        head = np.flatnonzero(np.r_[True, (np.diff(cols[0].astype(np.int64)) != 0)
                                    | (np.diff(fan) > R + 1)])
        a_ms, p_ms = float(np.median(host[1:])), float(np.median(floor[1:]))
        res = {"records": n, "shape": shape, "alignments": found[0], "path_records": found[1],
               "longest": int(got["n_words"].max()) if found[0] else 0,
               "segments_over_8": int((np.diff(np.r_[head, n]) > 8).sum()),
               "alignments_ms": round(a_ms, 3),
               "pass_ms": {name: round(float(np.median([p[k] for p in passes[1:]])), 3)
                           for k, name in enumerate(abi.ALIGNMENTS_MS_NAMES)},
               "passages_ms": round(p_ms, 3), "ratio": round(a_ms / p_ms, 2), "checked": False}
        k = min(n, args.oracle_records)
        if k:
            from tests import alignments_restated as ar
            part = [c[:k] for c in (cols[0], cols[1], cols[2], cols[4])]
            have, walk = alignments.find_alignments(*part, M, R, S, P, device=args.device)
            want, want_walk = ar.alignments(list(zip(*(c.tolist() for c in part))), M, R, S, P)
            assert len(want) == len(have) and walk.tolist() == want_walk
            for key in ar.KEYS:
                assert have[key].tolist() == [d[key] for d in want], key
            res["checked"] = True
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
