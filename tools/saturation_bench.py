#!/usr/bin/env python3
"""`saturation` timings, one JSON line per shape of the works and kind of unit:
  records       the four record mixes of tools/pairs_bench.py (small, medium, large, shared)
                over a 20 000-word script
  by            word: every script word inside a region of fs_quotes at --min-works 1; scene:
                300 scenes of equal length.  The unit map is made on the host and sits in HBM
                before the clock starts
  variants      the product's source of a work's time, FS_SATURATION_TABLE = 1 (`table`) and 0
                (`hash`), each with the shares of a unit row's words left to the library and
                forced to --ksplit (`table_split`, `hash_split`)
  <variant>_ms  fs_saturation_rows on those records already in HBM (median of --reps calls after
                a warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --permutations 1000 --points 100 --seed 0 --level 95, no first times out
  <variant>_event_ms
                the total of the HIP-event times of its passes (fs_saturation_times), median over
                the same calls.  The run heads (fs_passages.hip) and the host's waits make up
                the rest of <variant>_ms
  <variant>_incidence_ms, _sizes_ms, _times_ms, _product_ms, _curve_ms, _points_ms
                the passes, medians over the same calls; <variant>_product_spread_ms is the
                largest less the smallest product time of those calls
  <variant>_ksplit, <variant>_osplit
                the shares of a row's words and of its chunks of 64 orders the call took
  units, active, permutations, points, set_bits
                units; works with a passage; orders; points; set bits of the incidence matrix
                (the sum of works(u)): the product owes set_bits * permutations mins
  mins_per_s    set_bits * permutations over the product time of `table` and of `hash`
  intervals_ms, intervals_product_ms
                fs_intervals_rows on the same records and unit map in the same process, 1 000
                replicates, for scale
  same          the outputs of the four variants compared, every byte
  source        the hash of the library's sources the line was measured on (_lib.source_hash)
One line per row also goes to --out (default profiles/saturation_bench.jsonl).

usage: python tools/saturation_bench.py [--records N] [--reps R] [--permutations R]
           [--points K] [--ksplit S] [--shapes small,medium,large,shared] [--by word,scene]
           [--shared-works W] [--out profiles/saturation_bench.jsonl] [--device D]
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

from tools.pairs_bench import shared_records      # noqa: E402
from tools.works_bench import N_GROUPS, N_SCRIPT, records   # noqa: E402

PASSES = ("incidence_ms", "sizes_ms", "times_ms", "product_ms", "curve_ms", "points_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--permutations", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--ksplit", type=int, default=4)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--by", default="word,scene")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saturation_bench.jsonl"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    from fandom_search_amd import _lib, abi, quotes, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    L = _lib.load()
    dev = "cuda:%d" % args.device
    R, K = args.permutations, args.points
    variants = (("table", "1", None), ("hash", "0", None),
                ("table_split", "1", str(args.ksplit)), ("hash_split", "0", str(args.ksplit)))
    out = open(args.out, "w") if args.out else None
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        for by in args.by.split(","):
            if by == "word":
                qw, _ = quotes.find_quotes(*cols, np.zeros(n), n_works, N_SCRIPT, 6, 0, 1,
                                           args.device)
                at = np.nonzero(qw["region"] != abi.FS_NONE)[0]
                unit_of = np.full(N_SCRIPT, abi.FS_NONE, dtype=np.uint32)
                unit_of[at] = np.arange(len(at), dtype=np.uint32)
                n_units = len(at)
            else:
                unit_of = (np.arange(N_SCRIPT, dtype=np.uint32) * N_GROUPS // N_SCRIPT).astype(np.uint32)
                n_units = N_GROUPS
            d_map = torch.from_numpy(unit_of).to(dev)
            sizes = (max(1, n_units) * 4, K * abi.SATURATION_POINT_DTYPE.itemsize,
                     R * abi.SATURATION_PERM_DTYPE.itemsize,
                     abi.SATURATION_SUMMARY_DTYPE.itemsize)
            bufs = [torch.empty(s, dtype=torch.uint8, device=dev) for s in sizes]
            torch_ready()
            ptrs = tuple(b.data_ptr() for b in bufs)
            res = {"source": _lib.source_hash(), "records": n, "shape": shape, "by": by,
                   "works": n_works, "units": n_units, "permutations": R, "points": K,
                   "reps": args.reps}

            def call():
                ix.saturation_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                     permutations=R, points=K, out_ptrs=ptrs)
            seen = []
            for name, table, ksplit in variants:
                os.environ["FS_SATURATION_TABLE"] = table
                if ksplit is None:
                    os.environ.pop("FS_SATURATION_KSPLIT", None)
                else:
                    os.environ["FS_SATURATION_KSPLIT"] = ksplit
                call()                                                           # warm-up
                total, passes = [], []
                for _ in range(args.reps):
                    ms = (C.c_double * 10)()
                    t = time.perf_counter()
                    call()
                    total.append((time.perf_counter() - t) * 1e3)
                    L.fs_saturation_times(ms)
                    passes.append(list(ms))
                seen.append(tuple(b.cpu().numpy().tobytes() for b in bufs))
                res[name + "_ms"] = round(float(np.median(total)), 3)
                res[name + "_event_ms"] = round(float(np.median([p[6] for p in passes])), 3)
                for k, what in enumerate(PASSES):
                    res[name + "_" + what] = round(float(np.median([p[k] for p in passes])), 3)
                prod = [p[3] for p in passes]
                res[name + "_product_spread_ms"] = round(max(prod) - min(prod), 3)
                res[name + "_table"] = int(passes[-1][7])
                res[name + "_ksplit"] = int(passes[-1][8])
                res[name + "_osplit"] = int(passes[-1][9])
            os.environ.pop("FS_SATURATION_TABLE", None)
            os.environ.pop("FS_SATURATION_KSPLIT", None)
            res["same"] = all(s == seen[0] for s in seen[1:])
            works = np.frombuffer(seen[0][0], dtype=np.uint32)[:n_units]
            summary = np.frombuffer(seen[0][3], dtype=abi.SATURATION_SUMMARY_DTYPE)[0]
            res["active"] = int(summary["n_active"])
            res["units_quoted"] = int(summary["units_quoted"])
            res["set_bits"] = int(works.astype(np.int64).sum())
            for name in ("table", "hash"):
                ms = res[name + "_product_ms"]
                res[name + "_mins_per_s"] = float("%.3g" % (res["set_bits"] * R / (ms * 1e-3))) \
                    if ms > 0 else None
            # fs_intervals_rows beside it, for scale
            i_units = torch.empty(max(1, n_units) * abi.INTERVAL_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            i_reps = torch.empty(1000 * abi.INTERVAL_REPLICATE_DTYPE.itemsize, dtype=torch.uint8,
                                 device=dev)
            torch_ready()
            i_total, i_prod = [], []
            for k in range(args.reps + 1):
                ms = (C.c_double * 6)()
                t = time.perf_counter()
                ix.intervals_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                    replicates=1000, out_ptrs=(i_units.data_ptr(),
                                                               i_reps.data_ptr()))
                if k:
                    i_total.append((time.perf_counter() - t) * 1e3)
                    L.fs_intervals_times(ms)
                    i_prod.append(ms[2])
            res["intervals_ms"] = round(float(np.median(i_total)), 3)
            res["intervals_product_ms"] = round(float(np.median(i_prod)), 3)
            line = json.dumps(res)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
    if out:
        out.close()
    ix.close()


if __name__ == "__main__":
    main()
