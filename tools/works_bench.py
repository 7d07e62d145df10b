#!/usr/bin/env python3
"""`works` timings, one JSON line per shape of the works:
  records      N synthetic match records sorted by (work, fan_ix), the mix of
               tools/passages_bench.py over a 20 000-word script with 300 scenes
  shape        small: a new work every four records on average; medium: every thousand;
               large: ten works of N / 10 records
  works_ms     fs_works_rows on those records already in HBM (median of --reps calls after
               a warm-up, host clock around the synchronous call)
  passages_ms  fs_passages_rows on the same records, the same way: the new call does that
               work (the run heads) plus the reduction by work
  oracle_s     the test oracle (tests/works_restated.py) on the same records, up to
               --oracle-max records (its result is compared with the device's)
  works, cells what was found (--min-words 6, --max-gap 0)

usage: python tools/works_bench.py [--records N] [--reps R] [--shapes small,medium,large]
                                   [--oracle-max N] [--device D]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SCRIPT, N_GROUPS = 20_000, 300


def records(n, shape, seed=1):
    rng = np.random.default_rng(seed)
    if shape == "large":
        work = np.arange(n, dtype=np.int64) * 10 // n
    else:
        work = np.cumsum(rng.random(n) < (0.25 if shape == "small" else 1e-3))
    fstep = rng.choice([0, 1, 2], size=n, p=[0.02, 0.9, 0.08])
    fan = np.cumsum(fstep)
    ostep = np.where(rng.random(n) < 0.9, fstep, rng.integers(-40, 40, size=n))
    orig = (np.cumsum(ostep) + 40 * n + 1) % N_SCRIPT
    dist = rng.random(n) * 0.1
    comb = dist * rng.integers(0, 8, size=n)
    return (work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), dist, comb)


def median_ms(call, reps):
    call()                                             # warm-up
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(times)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large")
    ap.add_argument("--oracle-max", type=int, default=1_000_000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    n = args.records

    import torch
    from fandom_search_amd import abi, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    from fandom_search_amd.format import THRESHOLDS
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    group_of = (np.arange(N_SCRIPT, dtype=np.uint32) * N_GROUPS // N_SCRIPT).astype(np.uint32)
    dev = "cuda:%d" % args.device
    for shape in args.shapes.split(","):
        cols = records(n, shape)
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix", "dist", "comb"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        cap = min(n, n_works * N_GROUPS)
        d_out = torch.empty(n_works * abi.WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(n_works * (len(THRESHOLDS) + 1), dtype=torch.int32, device=dev)
        d_cells = torch.empty(cap * abi.WORK_CELL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pass = torch.empty((n // 6 + 1) * abi.PASSAGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        ptrs = (d_out.data_ptr(), d_counts.data_ptr(), d_cells.data_ptr())
        found = []
        works_ms = median_ms(lambda: found.append(ix.works_device(
            d_rows.data_ptr(), n, n_works, group_of, N_GROUPS, 6, 0, out_ptrs=ptrs, cap=cap)),
            args.reps)
        passages_ms = median_ms(lambda: ix.passages_device(
            d_rows.data_ptr(), n, 6, 0, out_ptr=d_pass.data_ptr(), cap=n // 6 + 1), args.reps)
        res = {"records": n, "shape": shape, "works": n_works, "cells": found[-1],
               "works_ms": works_ms, "passages_ms": passages_ms}
        if n <= args.oracle_max:
            from tests import works_restated
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = works_restated.works(recs, n_works, N_SCRIPT, group_of.tolist(), N_GROUPS, 6, 0)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            got = d_out.cpu().numpy().view(abi.WORK_DTYPE)
            assert len(want[2]) == found[-1]
            assert [int(x) for x in got["n_script_words"]] == [d["n_script_words"] for d in want[0]]
            assert [int(x) for x in got["passage_words"]] == [d["passage_words"] for d in want[0]]
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
