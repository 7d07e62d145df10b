#!/usr/bin/env python3
"""`retellings` timings, one JSON line per shape of the works:
  records        N synthetic match records sorted by (work, fan_ix): the three mixes of
                 tools/works_bench.py (small, medium, large), and `scrambled`: ten works of N / 10
                 records whose passages of eight words sit in shuffled script order, the
                 quadratic worst case of the large-work path
  retellings_ms  fs_retellings_rows on those records already in HBM (median of --reps calls
                 after a warm-up, host clock around the synchronous call)
  pass_ms        its passes by HIP events (fs_retellings_times), the median of each over the
                 same calls
  works_ms       fs_works_rows on the same records in the same process, the same way, for scale
  passages, max_passages   what was found (--min-words 6, --max-gap 0), and the most in a work
  checked        the result was compared with the test oracle (tests/retellings_restated.py);
                 done where no work has more than --oracle-max passages (the oracle is quadratic)

usage: python tools/retellings_bench.py [--records N] [--reps R]
                                        [--shapes small,medium,large,scrambled]
                                        [--oracle-max P] [--device D]
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

from works_bench import N_GROUPS, N_SCRIPT, records   # noqa: E402

WORDS = 8


def scrambled(n, seed=1):
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.int64)
    work = k * 10 // n
    fan = k + k // WORDS                                # a fan word skipped between two passages
    slot = rng.integers(0, N_SCRIPT // WORDS, size=n // WORDS + 1)
    orig = slot[k // WORDS] * WORDS + k % WORDS
    zero = np.zeros(n)
    return (work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), zero, zero)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,scrambled")
    ap.add_argument("--oracle-max", type=int, default=600)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    n = args.records

    import torch
    from fandom_search_amd import _lib, abi, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    from fandom_search_amd.format import THRESHOLDS
    L = _lib.load()
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    group_of = (np.arange(N_SCRIPT, dtype=np.uint32) * N_GROUPS // N_SCRIPT).astype(np.uint32)
    dev = "cuda:%d" % args.device
    for shape in args.shapes.split(","):
        cols = scrambled(n) if shape == "scrambled" else records(n, shape)
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix", "dist", "comb"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        cap_cells, cap = min(n, n_works * N_GROUPS), n // 6 + 1
        d_out = torch.empty(n_works * abi.WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_counts = torch.empty(n_works * (len(THRESHOLDS) + 1), dtype=torch.int32, device=dev)
        d_cells = torch.empty(cap_cells * abi.WORK_CELL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_tell = torch.empty(n_works * abi.RETELLING_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pass = torch.empty(cap * abi.RETELLING_PASSAGE_DTYPE.itemsize, dtype=torch.uint8,
                             device=dev)
        torch_ready()
        host, passes, found = [], [], 0
        ms = (C.c_double * 6)()
        for rep in range(args.reps + 1):                    # the first call is the warm-up
            t = time.perf_counter()
            found = ix.retellings_device(d_rows.data_ptr(), n, n_works, 6, 0,
                                         out_ptrs=(d_tell.data_ptr(), d_pass.data_ptr()), cap=cap)
            host.append((time.perf_counter() - t) * 1e3)
            L.fs_retellings_times(ms)
            passes.append(list(ms))
        works_t = []
        for rep in range(args.reps + 1):
            t = time.perf_counter()
            ix.works_device(d_rows.data_ptr(), n, n_works, group_of, N_GROUPS, 6, 0,
                            out_ptrs=(d_out.data_ptr(), d_counts.data_ptr(), d_cells.data_ptr()),
                            cap=cap_cells)
            works_t.append((time.perf_counter() - t) * 1e3)
        got_w = d_tell.cpu().numpy().view(abi.RETELLING_DTYPE)
        got_p = d_pass[:found * abi.RETELLING_PASSAGE_DTYPE.itemsize].cpu().numpy().view(
            abi.RETELLING_PASSAGE_DTYPE)
        most = int(got_w["n_passages"].max()) if n_works else 0
        res = {"records": n, "shape": shape, "works": n_works, "passages": found,
               "max_passages": most,
               "retellings_ms": round(float(np.median(host[1:])), 3),
               "pass_ms": {name: round(float(np.median([p[k] for p in passes[1:]])), 3)
                           for k, name in enumerate(abi.RETELLINGS_MS_NAMES)},
               "works_ms": round(float(np.median(works_t[1:])), 3), "checked": False}
        if most <= args.oracle_max:
            from tests import retellings_restated as rt
            want_w, want_p = rt.retellings(list(zip(*(c.tolist() for c in cols[:3]))), n_works, 6, 0)
            assert len(want_p) == found
            for key in rt.WORK_KEYS:
                assert got_w[key].tolist() == [d[key] for d in want_w], key
            for key in rt.PASSAGE_KEYS:
                assert got_p[key].tolist() == [d[key] for d in want_p], key
            res["checked"] = True
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
