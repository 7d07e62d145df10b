#!/usr/bin/env python3
"""`trends` timings, one JSON line per shape of the works and kind of unit:
  records       the four record mixes of tools/contrast_bench.py (small, medium, large, shared)
                over a 20 000-word script
  unit          word: every script word inside a region of fs_quotes at --min-works 1; scene:
                300 scenes of equal length.  The unit map and the period offsets are made on
                the host and sit in HBM before the clock starts.  The offsets spread the works
                over 240 months, (w * 2654435761 >> 7) % 240; every work is in the pool
  trends_ms     fs_trends_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-quoting 5 --permutations 1000 --seed 0, FS_TRENDS_MFMA unset
  pool_ms, labels_ms, product_ms, sweeps_ms
                HIP-event times of its passes (fs_trends_times), medians over the same calls.
                The run heads (fs_passages.hip) and the host's waits are inside pool_ms
  product_mfma_ms, product_plain_ms
                the product under FS_TRENDS_MFMA=1 and =0, the same way; `same` says the two
                settings wrote the same bytes
  units, active, permutations
                units; works with a passage; re-datings
  intervals_product_ms, product_over_intervals
                k_int_product of fs_intervals_rows on the same records, units and works at as
                many replicates, in the same process (fs_intervals_times, median of as many
                calls): one byte plane where the new product moves two for one expansion of M;
                product_mfma_ms over it
  restated      the units, the re-datings and the sums compared with tests/trends_restated.py
                on the records of the first --oracle-works works at --oracle-permutations
                re-datings, every field
  source        the hash of the library's sources the line was measured on (_lib.source_hash)
One line per row also goes to --out (default profiles/trends_bench.jsonl); the rows of the
README's table are printed behind them.

usage: python tools/trends_bench.py [--records N] [--reps R] [--permutations P]
           [--shapes small,medium,large,shared] [--unit word,scene] [--shared-works W]
           [--oracle-works 400] [--oracle-permutations 64]
           [--out profiles/trends_bench.jsonl] [--device D]
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

PASSES = ("pool_ms", "labels_ms", "product_ms", "sweeps_ms")
MONTHS = 240


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--permutations", type=int, default=1000)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--unit", default="word,scene")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-works", type=int, default=400)
    ap.add_argument("--oracle-permutations", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trends_bench.jsonl"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    from fandom_search_amd import _lib, abi, quotes, synth, trends
    from fandom_search_amd.companions import active_works
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    from tests import trends_restated as tr
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    L = _lib.load()
    dev = "cuda:%d" % args.device
    P = args.permutations
    out = open(args.out, "w") if args.out else None
    os.environ.pop("FS_TRENDS_MFMA", None)
    table = []
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        when = ((np.arange(n_works, dtype=np.int64) * 2654435761 >> 7) % MONTHS).astype(np.uint16)
        d_when = torch.from_numpy(when.view(np.int16)).to(dev)
        active = active_works(*cols, 6, 0)
        for unit in args.unit.split(","):
            if unit == "word":
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
            d_units = torch.empty(max(1, n_units) * abi.TRENDS_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            d_perms = torch.empty(P * abi.TRENDS_PERM_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            i_units = torch.empty(max(1, n_units) * abi.INTERVAL_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            i_reps = torch.empty(P * abi.INTERVAL_REPLICATE_DTYPE.itemsize, dtype=torch.uint8,
                                 device=dev)
            torch_ready()
            ptrs = (d_units.data_ptr(), d_perms.data_ptr())
            res = {"source": _lib.source_hash(), "records": n, "shape": shape, "unit": unit,
                   "works": n_works, "units": n_units, "active": active, "permutations": P,
                   "months": MONTHS, "reps": args.reps}

            def call():
                ix.trends_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                 d_when.data_ptr(), permutations=P, out_ptrs=ptrs)
            seen = []
            for mfma in (None, "1", "0"):
                if mfma is None:
                    os.environ.pop("FS_TRENDS_MFMA", None)
                else:
                    os.environ["FS_TRENDS_MFMA"] = mfma
                call()                                                     # warm-up
                total, passes = [], []
                for _ in range(args.reps):
                    ms = (C.c_double * 5)()
                    t = time.perf_counter()
                    call()
                    total.append((time.perf_counter() - t) * 1e3)
                    L.fs_trends_times(ms)
                    passes.append(list(ms))
                seen.append((d_units.cpu().numpy().tobytes(), d_perms.cpu().numpy().tobytes()))
                product = round(float(np.median([p[2] for p in passes])), 3)
                if mfma is None:
                    res["trends_ms"] = round(float(np.median(total)), 3)
                    for k, name in enumerate(PASSES):
                        res[name] = round(float(np.median([p[k] for p in passes])), 3)
                else:
                    res["product_mfma_ms" if mfma == "1" else "product_plain_ms"] = product
            os.environ.pop("FS_TRENDS_MFMA", None)
            res["same"] = seen[0] == seen[1] == seen[2]
            # the product of intervals on the same units and works, as many replicates
            ims, theirs = (C.c_double * 6)(), []
            for k in range(args.reps + 1):
                ix.intervals_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                    replicates=P, out_ptrs=(i_units.data_ptr(), i_reps.data_ptr()))
                L.fs_intervals_times(ims)
                if k:
                    theirs.append(ims[2])
            res["intervals_product_ms"] = round(float(np.median(theirs)), 3)
            res["product_over_intervals"] = \
                round(res["product_mfma_ms"] / res["intervals_product_ms"], 3) \
                if res["intervals_product_ms"] > 0 else None
            # the restatement on the first works
            few = min(args.oracle_works, n_works)
            keep = cols[0] < few
            sub = tuple(c[keep] for c in cols)
            t = time.perf_counter()
            want = tr.trends(list(zip(*(c.tolist() for c in sub))), few, N_SCRIPT,
                             unit_of.tolist(), n_units, when[:few].tolist(), 6, 0, 5,
                             args.oracle_permutations, 0)
            res["restated_s"] = round(time.perf_counter() - t, 3)
            got = trends.find_trends(*sub, few, N_SCRIPT, unit_of, n_units, when[:few], 6, 0, 5,
                                     args.oracle_permutations, 0, args.device, sums=True)
            ok = got[2].tolist() == want[2]
            for name in tr.UNIT_KEYS:
                ok = ok and got[0][name].tolist() == [d[name] for d in want[0]]
            for name in tr.PERM_KEYS:
                ok = ok and got[1][name].tolist() == [d[name] for d in want[1]]
            res["restated"] = bool(ok)
            line = json.dumps(res)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            table.append(res)
    if out:
        out.close()
    ix.close()
    print("| records | unit | units | active | trends | pool | labels | product (MFMA) | "
          "product (plain) | sweeps | `k_int_product` | product / `k_int_product` |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in table:
        print("| %s | %s | %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %s |"
              % (r["shape"], r["unit"], r["units"], r["active"], r["trends_ms"], r["pool_ms"],
                 r["labels_ms"], r["product_mfma_ms"], r["product_plain_ms"], r["sweeps_ms"],
                 r["intervals_product_ms"], r["product_over_intervals"]))


if __name__ == "__main__":
    main()
