#!/usr/bin/env python3
"""`routes` timings, one JSON line per shape of the works, kind of unit and skip, printed and
appended to --out (profiles/routes_bench.jsonl):
  records       the record mixes of tools/transitions_bench.py (small, medium, large, hot) over
                a 20 000-word script, and `planted`: works that each quote six of thirty
                stretches of eight words in a random order, half of them with one of ten planted
                routes of four stretches in its order, something else in between now and then
  by            region: the regions of fs_quotes at --min-works 1; scene: 300 scenes of equal
                length; units20: 20 units of equal length.  The unit map is made on the host and
                sits in HBM before the clock starts
  skip          --max-skip of the run: any distance, then 0
  routes_ms     fs_routes_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-all A --max-length K
  front_ms, tally_ms, passes_ms
                HIP-event times (fs_routes_times) of the sequence with the position tables and
                of the tally with the records, medians over the same calls; passes_ms is the
                total of all passes, the host's waits make up the rest
  levels        per length 2 .. K + 1: candidates, frequent, and join_ms, step_ms, count_ms,
                place_ms, mark_ms
  units, routes units; routes of 2 .. K units listed
  refused       the library's text when a level passes FS_ROUTES_MAX_SETS or the tables
                FS_ROUTES_MAX_BYTES: the case is then not timed
  transitions_ms, transitions_count_ms
                fs_transitions_rows on the same records and unit map in the same process, the
                same way (any distance, --min-steps 1 --min-step-works A --min-share 0), and its
                count pass
  not_run       the case was not started: --budget seconds had passed (0: no budget)
  oracle_s      the test oracle (tests/routes_restated.py) on the same records where it is
                affordable (up to --oracle-max records and --oracle-routes listed routes); its
                records are compared with the device's

usage: python tools/routes_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,hot,planted] [--by region,scene,units20] [--min-all A]
           [--max-length K] [--oracle-max N] [--oracle-routes S] [--budget SECONDS] [--out FILE]
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

from tools.transitions_bench import hot_records   # noqa: E402
from tools.works_bench import N_GROUPS, N_SCRIPT, records   # noqa: E402

STRETCHES, STRETCH_WORDS, PER_WORK, PLANTED, PLANTED_LENGTH = 30, 8, 6, 10, 4


def planted_records(n_records, seed=7):
    """Works that each quote PER_WORK of STRETCHES stretches in a random order, PLANTED planted
    routes of PLANTED_LENGTH stretches kept in their order."""
    rng = np.random.default_rng(seed)
    plants = [rng.choice(STRETCHES, size=PLANTED_LENGTH, replace=False).tolist()
              for _ in range(PLANTED)]
    n_works = max(1, n_records // (PER_WORK * STRETCH_WORDS))
    step = N_SCRIPT // STRETCHES
    run = np.arange(STRETCH_WORDS)
    work, fan, orig = [], [], []
    for w in range(n_works):
        order = list(plants[int(rng.integers(PLANTED))]) if rng.random() < 0.5 else []
        while len(order) < PER_WORK:
            s = int(rng.integers(STRETCHES))
            if s not in order:
                order.insert(int(rng.integers(0, len(order) + 1)), s)
        for k, s in enumerate(order):
            work.append(np.full(STRETCH_WORDS, w))
            fan.append(k * (STRETCH_WORDS + 10) + run)
            orig.append(s * step + run)
    return tuple(np.concatenate(c).astype(np.uint32) for c in (work, fan, orig))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,hot,planted")
    ap.add_argument("--by", default="region,scene,units20")
    ap.add_argument("--min-all", type=int, default=5)
    ap.add_argument("--max-length", type=int, default=4)
    ap.add_argument("--oracle-max", type=int, default=100_000)
    ap.add_argument("--oracle-routes", type=int, default=5000)
    ap.add_argument("--budget", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "routes_bench.jsonl"))
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
    a, k_max = args.min_all, args.max_length
    started = time.perf_counter()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def med(xs):
        return round(float(np.median(xs)), 3)

    for shape in args.shapes.split(","):
        if args.budget and time.perf_counter() - started > args.budget:
            emit({"shape": shape, "not_run": True})
            continue
        if shape == "hot":
            cols = hot_records(args.records)
        elif shape == "planted":
            cols = planted_records(args.records)
        else:
            cols = records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        for by in args.by.split(","):
            if args.budget and time.perf_counter() - started > args.budget:
                emit({"shape": shape, "by": by, "not_run": True})
                continue
            if by == "region":
                qw, qr = quotes.find_quotes(*cols, np.zeros(n), n_works, N_SCRIPT, 6, 0, 1,
                                            args.device)
                unit_of, n_units = np.ascontiguousarray(qw["region"]), len(qr)
            else:
                n_units = N_GROUPS if by == "scene" else 20
                unit_of = (np.arange(N_SCRIPT, dtype=np.uint32) * n_units // N_SCRIPT).astype(np.uint32)
            d_map = torch.from_numpy(unit_of).to(dev)
            torch_ready()
            base = (d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units, 6, 0)
            # fs_transitions_rows beside it, once per kind of unit
            t_units, t_cells = ix.transitions_device(*base, abi.FS_NONE, 1, a, 0)
            tcap = max(1, len(t_cells))
            d_tu = torch.empty(max(1, n_units) * abi.TRANSITION_UNIT_DTYPE.itemsize,
                               dtype=torch.uint8, device=dev)
            d_tc = torch.empty(tcap * abi.TRANSITION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch_ready()
            t_total, t_count = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 5)()
                t = time.perf_counter()
                ix.transitions_device(*base, abi.FS_NONE, 1, a, 0,
                                      out_ptrs=(d_tu.data_ptr(), d_tc.data_ptr()), cap=tcap)
                t_total.append((time.perf_counter() - t) * 1e3)
                L.fs_transitions_times(ms)
                t_count.append(ms[1])
            for skip in (abi.FS_NONE, 0):
                res = {"records": n, "shape": shape, "by": by, "works": n_works, "units": n_units,
                       "min_all": a, "max_length": k_max,
                       "skip": "any" if skip == abi.FS_NONE else skip}
                try:
                    h_units, h_levels, h_routes = ix.routes_device(*base, skip, a, k_max)  # warm-up
                except _lib.FsError as e:
                    if e.code != abi.FS_E_UNSUPPORTED:
                        raise
                    res["refused"] = str(e)
                    emit(res)
                    continue
                cap = max(1, len(h_routes))
                d_out = [torch.empty(max(1, c) * d.itemsize, dtype=torch.uint8, device=dev)
                         for c, d in ((n_units, abi.ROUTE_UNIT_DTYPE),
                                      (k_max, abi.ROUTE_LEVEL_DTYPE), (cap, abi.ROUTE_DTYPE))]
                torch_ready()
                ptrs = [t.data_ptr() for t in d_out]
                total, passes = [], []
                for _ in range(args.reps):
                    ms = (C.c_double * abi.FS_ROUTES_TIMES)()
                    t = time.perf_counter()
                    got = ix.routes_device(*base, skip, a, k_max, out_ptrs=ptrs, cap=cap)
                    total.append((time.perf_counter() - t) * 1e3)
                    L.fs_routes_times(ms)
                    passes.append(list(ms))
                res.update({"routes": got, "routes_ms": med(total),
                            "front_ms": med([p[0] for p in passes]),
                            "tally_ms": med([p[41] for p in passes]),
                            "passes_ms": med([p[42] for p in passes])})
                levels = []
                for v in h_levels:
                    length = int(v["length"])
                    at = 1 + 5 * (length - 2)
                    row = {"length": length, "candidates": int(v["candidates"]),
                           "frequent": int(v["frequent"])}
                    for j, name in enumerate(abi.ROUTES_LEVEL_MS_NAMES):
                        row[name + "_ms"] = med([p[at + j] for p in passes])
                    levels.append(row)
                res["levels"] = levels
                res["transitions_ms"] = med(t_total)
                res["transitions_count_ms"] = med(t_count)
                res["transitions_cells"] = len(t_cells)
                if n <= args.oracle_max and got <= args.oracle_routes:
                    from tests import routes_restated as rr
                    recs = list(zip(*(c.tolist() for c in cols)))
                    t = time.perf_counter()
                    want = rr.routes(recs, n_works, N_SCRIPT, unit_of.tolist(), n_units, 6, 0,
                                     skip, a, k_max)
                    res["oracle_s"] = round(time.perf_counter() - t, 3)
                    got_u = d_out[0].cpu().numpy().view(abi.ROUTE_UNIT_DTYPE)[:n_units]
                    got_l = d_out[1].cpu().numpy().view(abi.ROUTE_LEVEL_DTYPE)[:k_max]
                    got_r = d_out[2].cpu().numpy().view(abi.ROUTE_DTYPE)[:got]
                    assert len(want[2]) == got
                    for name in rr.UNIT_KEYS:
                        assert got_u[name].tolist() == [d[name] for d in want[0]], name
                    for name in rr.LEVEL_KEYS:
                        assert got_l[name].tolist() == [d[name] for d in want[1]], name
                    for name in rr.ROUTE_KEYS:
                        assert got_r[name].tolist() == [d[name] for d in want[2]], name
                emit(res)
    out.close()
    ix.close()


if __name__ == "__main__":
    main()
