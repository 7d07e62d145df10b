#!/usr/bin/env python3
"""`intervals` timings, one JSON line per shape of the works and kind of unit:
  records       the four record mixes of tools/pairs_bench.py (small, medium, large, shared)
                over a 20 000-word script
  by            word: every script word inside a region of fs_quotes at --min-works 1; scene:
                300 scenes of equal length.  The unit map is made on the host and sits in HBM
                before the clock starts
  intervals_ms  fs_intervals_rows on those records already in HBM (median of --reps calls after
                a warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --replicates 1000 --seed 0 --level 95, the product by MFMA
  incidence_ms, multiplicities_ms, product_ms, statistics_ms, neighbours_ms
                HIP-event times of its passes (fs_intervals_times), medians over the same
                calls.  The run heads (fs_passages.hip) and the host's waits make up the rest of
                intervals_ms
  plain_ms, product_plain_ms
                the call and its product pass under FS_INTERVALS_MFMA=0, the same way
  mfma_over_plain   product_ms / product_plain_ms, as measured
  units, active, replicates
                units; works with a passage; replicates
  macs_per_s    units * active * replicates multiply-adds, what the product owes before any
                padding, over product_ms; i8_peak_macs_per_s is the dense i8 MFMA rate of an
                MI355X beside it, 2.5e15 (twice the BF16 rate of about 2.5 PFLOP/s, two
                operations a multiply-add)
  companions_incidence_ms, companions_count_ms
                fs_companions_rows on the same records and unit map in the same process
                (--min-both 2), with no room for pairs, so that it ends behind its count pass:
                the same incidence matrix, and the unit x unit product on the vector ALUs
  same          the units and replicates of the two products compared, every byte
  source        the hash of the library's sources the line was measured on (_lib.source_hash)
One line per row also goes to --out (default profiles/intervals_bench.jsonl).

usage: python tools/intervals_bench.py [--records N] [--reps R] [--replicates B]
           [--shapes small,medium,large,shared] [--by word,scene] [--shared-works W]
           [--out profiles/intervals_bench.jsonl] [--device D]
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

PASSES = ("incidence_ms", "multiplicities_ms", "product_ms", "statistics_ms", "neighbours_ms")
I8_PEAK_MACS = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--by", default="word,scene")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intervals_bench.jsonl"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    from fandom_search_amd import _lib, abi, quotes, synth
    from fandom_search_amd.companions import active_works
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    L = _lib.load()
    dev = "cuda:%d" % args.device
    B = args.replicates
    out = open(args.out, "w") if args.out else None
    os.environ.pop("FS_INTERVALS_MFMA", None)
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
            d_units = torch.empty(max(1, n_units) * abi.INTERVAL_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            d_reps = torch.empty(B * abi.INTERVAL_REPLICATE_DTYPE.itemsize, dtype=torch.uint8,
                                 device=dev)
            torch_ready()
            ptrs = (d_units.data_ptr(), d_reps.data_ptr())
            res = {"source": _lib.source_hash(), "records": n, "shape": shape, "by": by,
                   "works": n_works, "units": n_units, "replicates": B, "reps": args.reps}
            seen = []
            for mfma in ("1", "0"):
                os.environ["FS_INTERVALS_MFMA"] = mfma
                ix.intervals_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                    replicates=B, out_ptrs=ptrs)                 # warm-up
                total, passes = [], []
                for _ in range(args.reps):
                    ms = (C.c_double * 6)()
                    t = time.perf_counter()
                    ix.intervals_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                        replicates=B, out_ptrs=ptrs)
                    total.append((time.perf_counter() - t) * 1e3)
                    L.fs_intervals_times(ms)
                    passes.append(list(ms))
                seen.append((d_units.cpu().numpy().tobytes(), d_reps.cpu().numpy().tobytes()))
                if mfma == "1":
                    res["intervals_ms"] = round(float(np.median(total)), 3)
                    for k, name in enumerate(PASSES):
                        res[name] = round(float(np.median([p[k] for p in passes])), 3)
                else:
                    res["plain_ms"] = round(float(np.median(total)), 3)
                    res["product_plain_ms"] = round(float(np.median([p[2] for p in passes])), 3)
            os.environ.pop("FS_INTERVALS_MFMA", None)
            got = np.frombuffer(seen[0][1], dtype=abi.INTERVAL_REPLICATE_DTYPE)
            res["units_quoted_most"] = int(got["units_quoted"].max())
            res["same"] = seen[0] == seen[1]
            # fs_companions_rows beside it: no room for pairs, so it ends behind the count pass
            cms = (C.c_double * 4)()
            c_units = torch.empty(max(1, n_units) * abi.COMPANION_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            torch_ready()
            c_inc, c_count = [], []
            for k in range(args.reps + 1):
                try:
                    ix.companions_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                         out_ptrs=(c_units.data_ptr(), 0), cap=0)
                except _lib.FsError as e:
                    if e.code != abi.FS_E_CAPACITY:
                        raise
                L.fs_companions_times(cms)
                if k:
                    c_inc.append(cms[0])
                    c_count.append(cms[1])
            res["companions_incidence_ms"] = round(float(np.median(c_inc)), 3)
            res["companions_count_ms"] = round(float(np.median(c_count)), 3)
            res["active"] = active_works(*cols, 6, 0)
            macs = n_units * res["active"] * B
            res["macs_per_s"] = float("%.3g" % (macs / (res["product_ms"] * 1e-3))) \
                if res["product_ms"] > 0 else None
            res["i8_peak_macs_per_s"] = I8_PEAK_MACS
            res["mfma_over_plain"] = round(res["product_ms"] / res["product_plain_ms"], 3) \
                if res["product_plain_ms"] > 0 else None
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
