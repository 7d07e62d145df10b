#!/usr/bin/env python3
"""`transitions` timings, one JSON line per shape of the works and kind of unit:
  records       the three record mixes of tools/works_bench.py (small, medium, large) over a
                20 000-word script, and `hot`: works of 25 passages of six words, every passage
                at one of two places of the script, so that every step lands in one of 4 cells
  by            region: the regions of fs_quotes at --min-works 1; scene: 300 scenes of equal
                length (the hashed class); units20: 20 units of equal length (the dense class).
                The unit map is made on the host and sits in HBM before the clock starts
  transitions_ms  fs_transitions_rows on those records already in HBM (median of --reps calls
                after a warm-up, host clock around the synchronous call), --min-words 6
                --max-gap 0, any distance, --min-steps 1 --min-step-works 2 --min-share 0
  sequence_ms, count_ms, keep_ms, place_ms, total_ms
                HIP-event times of its passes (fs_transitions_times), medians over the same
                calls, and count_spread: the least and the largest count_ms of them
  hashed_count_ms, hashed_ms, dense_speedup
                where the call takes the dense class: the same calls under
                FS_TRANSITIONS_DENSE=0, the same counting through per-step global atomics; and
                hashed_count_ms / count_ms
  retellings_ms, retellings_passages_ms
                fs_retellings_rows on the same records in the same process, the same way, and
                its passages pass: the shared front end (checks, run heads, kept runs)
  companions_ms fs_companions_rows on the same records and unit map (--min-both 2)
  units, sequence, cells
                units; unit-bearing passages (the sum of the units' passages); cells kept
  oracle_s      the test oracle (tests/transitions_restated.py) on the same records where it
                takes a few seconds (up to --oracle-max records); its result is compared with
                the device's

usage: python tools/transitions_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,hot] [--by region,scene,units20] [--oracle-max N]
           [--device D]
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

from tools.works_bench import N_GROUPS, N_SCRIPT, records   # noqa: E402

PASSES = ("sequence_ms", "count_ms", "keep_ms", "place_ms", "total_ms")
HOT_WORDS, HOT_PASSAGES, HOT_GAP = 6, 25, 3


def hot_records(n, seed=1):
    """n records (a multiple of six below it): passages of six words at script word 0 or at the
    script's middle, 25 to a work, three fan words between two of them."""
    rng = np.random.default_rng(seed)
    n_pass = n // HOT_WORDS
    p = np.repeat(np.arange(n_pass, dtype=np.int64), HOT_WORDS)
    k = np.tile(np.arange(HOT_WORDS, dtype=np.int64), n_pass)
    at = rng.integers(0, 2, n_pass) * (N_SCRIPT // 2)
    work = p // HOT_PASSAGES
    fan = (p % HOT_PASSAGES) * (HOT_WORDS + HOT_GAP) + k
    return work.astype(np.uint32), fan.astype(np.uint32), (at[p] + k).astype(np.uint32)


def timed(L, call, reps):
    """Medians over reps calls: (host ms, [pass ms], (least, largest count ms))."""
    total, passes = [], []
    for _ in range(reps):
        ms = (C.c_double * 5)()
        t = time.perf_counter()
        call()
        total.append((time.perf_counter() - t) * 1e3)
        L.fs_transitions_times(ms)
        passes.append(list(ms))
    count = [p[1] for p in passes]
    return (round(float(np.median(total)), 3),
            [round(float(np.median([p[k] for p in passes])), 3) for k in range(5)],
            (round(min(count), 3), round(max(count), 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,hot")
    ap.add_argument("--by", default="region,scene,units20")
    ap.add_argument("--oracle-max", type=int, default=200_000)
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
    os.environ.pop("FS_TRANSITIONS_DENSE", None)
    for shape in args.shapes.split(","):
        cols = hot_records(args.records) if shape == "hot" else records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        # fs_retellings_rows beside it, once per shape
        _, host_pass = ix.retellings_device(d_rows.data_ptr(), n, n_works)
        rcap = max(1, len(host_pass))
        d_rw = torch.empty(n_works * abi.RETELLING_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_rp = torch.empty(rcap * abi.RETELLING_PASSAGE_DTYPE.itemsize, dtype=torch.uint8,
                           device=dev)
        torch_ready()
        r_total, r_pass = [], []
        for _ in range(args.reps):
            ms = (C.c_double * 6)()
            t = time.perf_counter()
            ix.retellings_device(d_rows.data_ptr(), n, n_works,
                                 out_ptrs=(d_rw.data_ptr(), d_rp.data_ptr()), cap=rcap)
            r_total.append((time.perf_counter() - t) * 1e3)
            L.fs_retellings_times(ms)
            r_pass.append(ms[0])
        for by in args.by.split(","):
            if by == "region":
                qw, qr = quotes.find_quotes(*cols, np.zeros(n), n_works, N_SCRIPT, 6, 0, 1,
                                            args.device)
                unit_of, n_units = np.ascontiguousarray(qw["region"]), len(qr)
            else:
                n_units = N_GROUPS if by == "scene" else 20
                unit_of = (np.arange(N_SCRIPT, dtype=np.uint32) * n_units // N_SCRIPT).astype(np.uint32)
            d_map = torch.from_numpy(unit_of).to(dev)
            torch_ready()
            host_units, host_cells = ix.transitions_device(d_rows.data_ptr(), n, n_works,
                                                           d_map.data_ptr(), n_units)   # warm-up
            cap = max(1, len(host_cells))
            d_units = torch.empty(max(1, n_units) * abi.TRANSITION_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            d_cells = torch.empty(cap * abi.TRANSITION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch_ready()
            ptrs = (d_units.data_ptr(), d_cells.data_ptr())

            def call():
                return ix.transitions_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(),
                                             n_units, out_ptrs=ptrs, cap=cap)
            total, passes, spread = timed(L, call, args.reps)
            res = {"records": n, "shape": shape, "by": by, "works": n_works, "units": n_units,
                   "sequence": int(host_units["passages"].sum()), "cells": len(host_cells),
                   "steps": int(host_units["steps_out"].sum()),
                   "class": "dense" if n_units <= abi.FS_TRANSITIONS_DENSE else "hashed",
                   "transitions_ms": total}
            res.update(zip(PASSES, passes))
            res["count_spread"] = spread
            if n_units <= abi.FS_TRANSITIONS_DENSE:
                os.environ["FS_TRANSITIONS_DENSE"] = "0"
                call()                                                  # warm-up
                h_total, h_passes, h_spread = timed(L, call, args.reps)
                os.environ.pop("FS_TRANSITIONS_DENSE")
                got = (d_units.cpu().numpy().view(abi.TRANSITION_UNIT_DTYPE)[:n_units],
                       d_cells.cpu().numpy().view(abi.TRANSITION_DTYPE)[:len(host_cells)])
                assert (got[0] == host_units).all() and (got[1] == host_cells).all()
                res["hashed_ms"], res["hashed_count_ms"] = h_total, h_passes[1]
                res["hashed_count_spread"] = h_spread
                res["dense_speedup"] = round(h_passes[1] / passes[1], 2) if passes[1] > 0 else None
            res["retellings_ms"] = round(float(np.median(r_total)), 3)
            res["retellings_passages_ms"] = round(float(np.median(r_pass)), 3)
            ccap = max(1, len(ix.companions_device(d_rows.data_ptr(), n, n_works,
                                                   d_map.data_ptr(), n_units)[1]))
            d_cu = torch.empty(max(1, n_units) * abi.COMPANION_UNIT_DTYPE.itemsize,
                               dtype=torch.uint8, device=dev)
            d_cp = torch.empty(ccap * abi.COMPANION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch_ready()
            c_total = []
            for _ in range(args.reps):
                t = time.perf_counter()
                ix.companions_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                     out_ptrs=(d_cu.data_ptr(), d_cp.data_ptr()), cap=ccap)
                c_total.append((time.perf_counter() - t) * 1e3)
            res["companions_ms"] = round(float(np.median(c_total)), 3)
            if n <= args.oracle_max:
                from tests import transitions_restated as tr
                recs = list(zip(*(c.tolist() for c in cols)))
                t = time.perf_counter()
                want = tr.transitions(recs, n_works, N_SCRIPT, unit_of.tolist(), n_units, 6, 0)
                res["oracle_s"] = round(time.perf_counter() - t, 3)
                assert len(want[1]) == len(host_cells)
                for name in tr.UNIT_KEYS:
                    assert host_units[name].tolist() == [d[name] for d in want[0]], name
                for name in tr.CELL_KEYS:
                    assert host_cells[name].tolist() == [d[name] for d in want[1]], name
            print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
