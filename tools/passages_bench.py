#!/usr/bin/env python3
"""`passages` timings, one JSON line:
  records      N synthetic match records, sorted by (work, fan_ix), mostly diagonal runs
  rows_ms      fs_passages_rows on those records already in HBM (median of --reps calls,
               host clock around the synchronous call)
  command_s    `python ao3.py passages` end to end on a match CSV of the same N records
               (a fresh process: read, sort, fs_passages, write)
  oracle_s     the test oracle (tests/passages_restated.py) on the same records
  passages     passages found (--min-words 6, --max-gap 0)

usage: python tools/passages_bench.py [--records N] [--reps R] [--device D]
"""

import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def records(n, seed=1):
    rng = np.random.default_rng(seed)
    work = np.cumsum(rng.random(n) < 1e-3)
    fstep = rng.choice([0, 1, 2], size=n, p=[0.02, 0.9, 0.08])
    fan = np.cumsum(fstep)
    ostep = np.where(rng.random(n) < 0.9, fstep, rng.integers(-40, 40, size=n))
    orig = np.cumsum(ostep) + 40 * n + 1
    dist = rng.random(n) * 0.1
    comb = dist * rng.integers(0, 8, size=n)
    return (work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), dist, comb)


def write_csv(path, cols):
    work, fan, orig, dist, comb = cols
    with open(path, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh)
        for k in range(len(work)):
            o = int(orig[k])
            w.writerow(["w%07d.txt" % work[k], int(fan[k]), "f%d" % (o % 997), 1, o,
                        "s%d" % (o % 991), 2, "ANNA", 1, float(dist[k]), 3, float(comb[k])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    n = args.records
    cols = records(n)

    import torch
    from fandom_search_amd import abi, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    words = synth.vocab_words()
    script = synth.script_tokens(2000)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    rows = np.zeros(n, dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix", "dist", "comb"), cols):
        rows[name] = col
    d_rows = torch.from_numpy(rows.view(np.uint8)).to("cuda:%d" % args.device)
    cap = n // 6 + 1
    d_out = torch.empty(cap * abi.PASSAGE_DTYPE.itemsize, dtype=torch.uint8, device=d_rows.device)
    torch_ready()
    found = ix.passages_device(d_rows.data_ptr(), n, 6, 0, out_ptr=d_out.data_ptr(), cap=cap)  # warm
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        ix.passages_device(d_rows.data_ptr(), n, 6, 0, out_ptr=d_out.data_ptr(), cap=cap)
        times.append((time.perf_counter() - t) * 1e3)
    ix.close()

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "match.csv")
        write_csv(path, cols)
        t = time.perf_counter()
        subprocess.check_call([sys.executable, os.path.join(ROOT, "ao3.py"), "passages", path,
                               "--device", str(args.device)])
        command_s = time.perf_counter() - t
        with open(os.path.join(tmp, "match-passages.csv")) as fh:
            assert sum(1 for _ in fh) == found + 1

    from tests import passages_restated
    recs = list(zip(*(c.tolist() for c in cols)))
    t = time.perf_counter()
    want = passages_restated.passages(recs, 6, 0)
    oracle_s = time.perf_counter() - t
    assert len(want) == found
    print(json.dumps({"records": n, "rows_ms": round(float(np.median(times)), 3),
                      "command_s": round(command_s, 3), "oracle_s": round(oracle_s, 3),
                      "passages": found}))


if __name__ == "__main__":
    main()
