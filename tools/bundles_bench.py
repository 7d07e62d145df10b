#!/usr/bin/env python3
"""`bundles` timings, one JSON line per shape of the works, kind of unit and pruning switch,
printed and appended to --out (profiles/bundles_bench.jsonl):
  records       the four record mixes of tools/companions_bench.py (small, medium, large,
                shared) over a 20 000-word script, and `packs`: works that each quote six of
                thirty stretches of eight words, half of them one of ten planted packs of four
                stretches and two others
  by            region: the regions of fs_quotes at --min-works 1; scene: 300 scenes of equal
                length.  The unit map is made on the host and sits in HBM before the clock starts
  prune         FS_BUNDLES_PRUNE of the run: every case runs with 1, then once more with 0
  bundles_ms    fs_bundles_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-all A --max-size K
  incidence_ms, level2_ms, tally_ms, passes_ms
                HIP-event times of its passes (fs_bundles_times), medians over the same calls;
                passes_ms is their total, the run heads and the host's waits make up the rest
  levels        per size 3 .. K + 1: candidates, frequent, and join_ms, count_ms, place_ms,
                mark_ms; word_ands_per_s is (candidates + parents * (size - 1)) * ceil(active / 64)
                64-bit ANDs, what an unpruned count pass owes, over count_ms
  units, active, sets
                units; works with a passage; sets of 2 .. K units listed
  refused       the library's text when a level passes FS_BUNDLES_MAX_SETS or the tables
                FS_BUNDLES_MAX_BYTES: the case is then not timed
  companions_ms, companions_count_ms
                fs_companions_rows on the same records in the same process, the same way, at
                --min-both A, and its count pass: level 2 is that product
  oracle_s      the test oracle (tests/bundles_restated.py) on the same records where it is
                affordable (up to --oracle-max active works, --oracle-units units and
                --oracle-sets listed sets); its records are compared with the device's

usage: python tools/bundles_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,shared,packs] [--by region,scene] [--min-all A]
           [--max-size K] [--shared-works W] [--oracle-max A] [--oracle-units U]
           [--oracle-sets S] [--out FILE] [--device D]
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

STRETCHES, STRETCH_WORDS, PER_WORK, PACKS, PACK_SIZE = 30, 8, 6, 10, 4


def packs_records(n_records, seed=7):
    """Works that each quote PER_WORK of STRETCHES stretches, PACKS planted packs of
    PACK_SIZE."""
    rng = np.random.default_rng(seed)
    packs = [rng.choice(STRETCHES, size=PACK_SIZE, replace=False) for _ in range(PACKS)]
    n_works = max(1, n_records // (PER_WORK * STRETCH_WORDS))
    step = N_SCRIPT // STRETCHES
    run = np.arange(STRETCH_WORDS)
    work, fan, orig = [], [], []
    for w in range(n_works):
        mine = set()
        if rng.random() < 0.5:
            mine |= set(packs[int(rng.integers(PACKS))].tolist())
        while len(mine) < PER_WORK:
            mine.add(int(rng.integers(STRETCHES)))
        for k, s in enumerate(sorted(mine)):
            work.append(np.full(STRETCH_WORDS, w))
            fan.append(k * (STRETCH_WORDS + 10) + run)
            orig.append(s * step + run)
    return tuple(np.concatenate(c).astype(np.uint32) for c in (work, fan, orig))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared,packs")
    ap.add_argument("--by", default="region,scene")
    ap.add_argument("--min-all", type=int, default=5)
    ap.add_argument("--max-size", type=int, default=4)
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-max", type=int, default=4000)
    ap.add_argument("--oracle-units", type=int, default=400)
    ap.add_argument("--oracle-sets", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundles_bench.jsonl"))
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
    a, k_max = args.min_all, args.max_size
    out = open(args.out, "a")

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def med(xs):
        return round(float(np.median(xs)), 3)

    for shape in args.shapes.split(","):
        if shape == "shared":
            cols = shared_records(args.shared_works)
        elif shape == "packs":
            cols = packs_records(args.records)
        else:
            cols = records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
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
            base = (d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units, 6, 0)
            # fs_companions_rows beside it, once per kind of unit
            c_units, c_found = ix.companions_device(*base, a, 0)
            ccap = max(1, len(c_found))
            d_cu = torch.empty(max(1, n_units) * abi.COMPANION_UNIT_DTYPE.itemsize,
                               dtype=torch.uint8, device=dev)
            d_cf = torch.empty(ccap * abi.COMPANION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            torch_ready()
            c_total, c_count = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 4)()
                t = time.perf_counter()
                ix.companions_device(*base, a, 0, out_ptrs=(d_cu.data_ptr(), d_cf.data_ptr()),
                                     cap=ccap)
                c_total.append((time.perf_counter() - t) * 1e3)
                L.fs_companions_times(ms)
                c_count.append(ms[1])
            for prune in (1, 0):
                os.environ["FS_BUNDLES_PRUNE"] = str(prune)
                res = {"records": n, "shape": shape, "by": by, "works": n_works, "units": n_units,
                       "min_all": a, "max_size": k_max, "prune": prune}
                try:
                    h_units, h_levels, h_sets = ix.bundles_device(*base, a, k_max)   # warm-up
                except _lib.FsError as e:
                    if e.code != abi.FS_E_UNSUPPORTED:
                        raise
                    res["refused"] = str(e)
                    emit(res)
                    continue
                cap = max(1, len(h_sets))
                d_out = [torch.empty(max(1, c) * d.itemsize, dtype=torch.uint8, device=dev)
                         for c, d in ((n_units, abi.BUNDLE_UNIT_DTYPE),
                                      (k_max, abi.BUNDLE_LEVEL_DTYPE), (cap, abi.BUNDLE_DTYPE))]
                torch_ready()
                ptrs = [t.data_ptr() for t in d_out]
                total, passes = [], []
                for _ in range(args.reps):
                    ms = (C.c_double * abi.FS_BUNDLES_TIMES)()
                    t = time.perf_counter()
                    got = ix.bundles_device(*base, a, k_max, out_ptrs=ptrs, cap=cap)
                    total.append((time.perf_counter() - t) * 1e3)
                    L.fs_bundles_times(ms)
                    passes.append(list(ms))
                active = active_works(*cols, 6, 0)
                res.update({"active": active, "sets": got, "bundles_ms": med(total),
                            "incidence_ms": med([p[0] for p in passes]),
                            "level2_ms": med([p[1] for p in passes]),
                            "tally_ms": med([p[30] for p in passes]),
                            "passes_ms": med([p[31] for p in passes])})
                levels = []
                for v in h_levels[1:]:
                    s = int(v["size"])
                    at = 2 + 4 * (s - 3)
                    row = {"size": s, "candidates": int(v["candidates"]),
                           "frequent": int(v["frequent"])}
                    for j, name in enumerate(abi.BUNDLES_LEVEL_MS_NAMES):
                        row[name + "_ms"] = med([p[at + j] for p in passes])
                    parents = int(h_levels[s - 3]["frequent"])
                    ands = (row["candidates"] + parents * (s - 1)) * ((active + 63) // 64)
                    row["word_ands_per_s"] = float("%.3g" % (ands / (row["count_ms"] * 1e-3))) \
                        if row["count_ms"] > 0 else None
                    levels.append(row)
                res["levels"] = levels
                res["companions_ms"] = med(c_total)
                res["companions_count_ms"] = med(c_count)
                res["companions_pairs"] = len(c_found)
                if (active <= args.oracle_max and n_units <= args.oracle_units
                        and got <= args.oracle_sets):
                    from tests import bundles_restated as br
                    recs = list(zip(*(c.tolist() for c in cols)))
                    t = time.perf_counter()
                    want = br.bundles(recs, n_works, N_SCRIPT, unit_of.tolist(), n_units, 6, 0, a,
                                      k_max)
                    res["oracle_s"] = round(time.perf_counter() - t, 3)
                    got_u = d_out[0].cpu().numpy().view(abi.BUNDLE_UNIT_DTYPE)[:n_units]
                    got_l = d_out[1].cpu().numpy().view(abi.BUNDLE_LEVEL_DTYPE)[:k_max]
                    got_s = d_out[2].cpu().numpy().view(abi.BUNDLE_DTYPE)[:got]
                    assert len(want[2]) == got
                    for name in br.UNIT_KEYS:
                        assert got_u[name].tolist() == [d[name] for d in want[0]], name
                    for name in br.LEVEL_KEYS:
                        assert got_l[name].tolist() == [d[name] for d in want[1]], name
                    for name in br.SET_KEYS:
                        assert got_s[name].tolist() == [d[name] for d in want[2]], name
                emit(res)
            os.environ.pop("FS_BUNDLES_PRUNE", None)
    out.close()
    ix.close()


if __name__ == "__main__":
    main()
