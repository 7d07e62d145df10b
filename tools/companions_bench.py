#!/usr/bin/env python3
"""`companions` timings, one JSON line per shape of the works and kind of unit:
  records       the four record mixes of tools/pairs_bench.py (small, medium, large, shared)
                over a 20 000-word script
  by            region: the regions of fs_quotes at --min-works 1; scene: 300 scenes of equal
                length.  The unit map is made on the host and sits in HBM before the clock starts
  companions_ms fs_companions_rows on those records already in HBM (median of --reps calls after
                a warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-both 2 --min-share 0
  incidence_ms, count_ms, place_ms, detail_ms
                HIP-event times of its passes (fs_companions_times), medians over the same
                calls: the incidence matrix with the row popcounts; the count pass with its
                scan and the per-unit results; the place pass; the detail pass.  The run heads
                (fs_passages.hip) and the host's waits make up the rest of companions_ms
  units, active, pairs
                units; works with a passage; pairs kept
  word_ands_per_s   units * (units - 1) / 2 * ceil(active / 64) 64-bit ANDs, what the count
                pass owes, over count_ms
  pairs_ms, pairs_count_ms
                fs_pairs_rows on the same records in the same process, the same way, and its
                count pass (--min-shared 6): the same tile product with rows of
                ceil(script / 64) words
  oracle_s      the test oracle (tests/companions_restated.py) on the same records where it is
                affordable (up to --oracle-max active works and --oracle-units units); its
                result is compared with the device's

usage: python tools/companions_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,shared] [--by region,scene] [--shared-works W]
           [--oracle-max A] [--oracle-units U] [--device D]
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

PASSES = ("incidence_ms", "count_ms", "place_ms", "detail_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--by", default="region,scene")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-max", type=int, default=4000)
    ap.add_argument("--oracle-units", type=int, default=1500)
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
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        # fs_pairs_rows beside it, once per shape
        host_works, host_pairs = ix.pairs_device(d_rows.data_ptr(), n, n_works)
        active = int((host_works["covered"] > 0).sum())
        pcap = max(1, len(host_pairs))
        d_pw = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pp = torch.empty(pcap * abi.PAIR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        p_total, p_count = [], []
        for _ in range(args.reps):
            ms = (C.c_double * 4)()
            t = time.perf_counter()
            ix.pairs_device(d_rows.data_ptr(), n, n_works, out_ptrs=(d_pw.data_ptr(), d_pp.data_ptr()),
                            cap=pcap)
            p_total.append((time.perf_counter() - t) * 1e3)
            L.fs_pairs_times(ms)
            p_count.append(ms[1])
        for by in args.by.split(","):
            if by == "region":
                qw, qr = quotes.find_quotes(*cols, np.zeros(n), n_works, N_SCRIPT, 6, 0, 1,
                                            args.device)
                unit_of, n_units = np.ascontiguousarray(qw["region"]), len(qr)
            else:
                unit_of = (np.arange(N_SCRIPT, dtype=np.uint32) * N_GROUPS // N_SCRIPT).astype(np.uint32)
                n_units = N_GROUPS
            d_map = torch.from_numpy(unit_of).to(dev)
            torch_ready()
            host_units, host_found = ix.companions_device(d_rows.data_ptr(), n, n_works,
                                                          d_map.data_ptr(), n_units)   # warm-up
            cap = max(1, len(host_found))
            d_units = torch.empty(max(1, n_units) * abi.COMPANION_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            d_found = torch.empty(cap * abi.COMPANION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch_ready()
            ptrs = (d_units.data_ptr(), d_found.data_ptr())
            total, passes = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 4)()
                t = time.perf_counter()
                got = ix.companions_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                           out_ptrs=ptrs, cap=cap)
                total.append((time.perf_counter() - t) * 1e3)
                L.fs_companions_times(ms)
                passes.append(list(ms))
            res = {"records": n, "shape": shape, "by": by, "works": n_works, "active": active,
                   "units": n_units, "pairs": got,
                   "companions_ms": round(float(np.median(total)), 3)}
            for k, name in enumerate(PASSES):
                res[name] = round(float(np.median([p[k] for p in passes])), 3)
            ands = n_units * (n_units - 1) // 2 * ((active + 63) // 64)
            res["word_ands_per_s"] = float("%.3g" % (ands / (res["count_ms"] * 1e-3))) \
                if res["count_ms"] > 0 else None
            res["pairs_ms"] = round(float(np.median(p_total)), 3)
            res["pairs_count_ms"] = round(float(np.median(p_count)), 3)
            res["pairs_pairs"] = len(host_pairs)
            if active <= args.oracle_max and n_units <= args.oracle_units:
                from tests import companions_restated as cr
                recs = list(zip(*(c.tolist() for c in cols)))
                t = time.perf_counter()
                want = cr.companions(recs, n_works, N_SCRIPT, unit_of.tolist(), n_units, 6, 0, 2, 0)
                res["oracle_s"] = round(time.perf_counter() - t, 3)
                got_u = d_units.cpu().numpy().view(abi.COMPANION_UNIT_DTYPE)[:n_units]
                got_p = d_found.cpu().numpy().view(abi.COMPANION_DTYPE)[:got]
                assert len(want[1]) == got
                for name in cr.UNIT_KEYS:
                    assert got_u[name].tolist() == [d[name] for d in want[0]], name
                for name in cr.PAIR_KEYS:
                    assert got_p[name].tolist() == [d[name] for d in want[1]], name
            print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
