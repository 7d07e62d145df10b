#!/usr/bin/env python3
"""`quotes` timings, one JSON line per shape of the works:
  records      N synthetic match records sorted by (work, fan_ix), the mixes of
               tools/works_bench.py over a 20 000-word script
  shape        small: a new work every four records on average; medium: every thousand;
               large: ten works of N / 10 records
  quotes_ms    fs_quotes_rows on those records already in HBM (median of --reps calls after a
               warm-up, host clock around the synchronous call), --min-works 1 and
               quotes2_ms at --min-works 2
  passages_ms  fs_passages_rows on the same records, the same way: the new call does that
  works_ms     work (the run heads) plus its own; fs_works_rows with 300 scenes likewise
  oracle_s     the test oracle (tests/quotes_restated.py) on the same records, up to
               --oracle-max records (its result is compared with the device's)
  regions      what was found (--min-words 6, --max-gap 0), at one work and at two

usage: python tools/quotes_bench.py [--records N] [--reps R] [--shapes small,medium,large]
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

from tools.works_bench import N_GROUPS, N_SCRIPT, median_ms, records   # noqa: E402


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
        rcap = N_SCRIPT // 2
        d_words = torch.empty(N_SCRIPT * abi.QUOTE_WORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_regions = torch.empty(rcap * abi.QUOTE_REGION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_out = torch.empty(n_works * abi.WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(n_works * (len(THRESHOLDS) + 1), dtype=torch.int32, device=dev)
        d_cells = torch.empty(cap * abi.WORK_CELL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pass = torch.empty((n // 6 + 1) * abi.PASSAGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        qptrs = (d_words.data_ptr(), d_regions.data_ptr())
        wptrs = (d_out.data_ptr(), d_counts.data_ptr(), d_cells.data_ptr())
        found = {}
        res = {"records": n, "shape": shape, "works": n_works}
        for k, key in ((2, "quotes2_ms"), (1, "quotes_ms")):
            res[key] = median_ms(lambda: found.__setitem__(k, ix.quotes_device(
                d_rows.data_ptr(), n, n_works, 6, 0, k, out_ptrs=qptrs, cap=rcap)), args.reps)
        res["regions"], res["regions2"] = found[1], found[2]
        res["passages_ms"] = median_ms(lambda: ix.passages_device(
            d_rows.data_ptr(), n, 6, 0, out_ptr=d_pass.data_ptr(), cap=n // 6 + 1), args.reps)
        res["works_ms"] = median_ms(lambda: ix.works_device(
            d_rows.data_ptr(), n, n_works, group_of, N_GROUPS, 6, 0, out_ptrs=wptrs, cap=cap),
            args.reps)
        if n <= args.oracle_max:
            from tests import quotes_restated
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = quotes_restated.quotes(recs, n_works, N_SCRIPT, 6, 0, 1)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            got_w = d_words.cpu().numpy().view(abi.QUOTE_WORD_DTYPE)
            got_r = d_regions.cpu().numpy().view(abi.QUOTE_REGION_DTYPE)[:found[1]]
            assert len(want[1]) == found[1]
            for name in quotes_restated.WORD_KEYS:
                assert got_w[name].tolist() == [d[name] for d in want[0]], name
            for name in quotes_restated.REGION_KEYS:
                assert got_r[name].tolist() == [d[name] for d in want[1]], name
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
