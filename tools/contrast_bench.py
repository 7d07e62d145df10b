#!/usr/bin/env python3
"""`contrast` timings, one JSON line per shape of the works and kind of unit:
  records       the four record mixes of tools/pairs_bench.py (small, medium, large, shared)
                over a 20 000-word script
  unit          word: every script word inside a region of fs_quotes at --min-works 1; scene:
                300 scenes of equal length.  The unit map and the side bytes are made on the
                host and sit in HBM before the clock starts.  Side A is every work whose number
                is below a third of the works, side B every other work
  contrast_ms   fs_contrast_rows on those records already in HBM (median of --reps calls after
                a warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-quoting 5 --permutations 1000 --seed 0, key_bits 32
  incidence_ms, selection_ms, product_ms, sweeps_ms
                HIP-event times of its passes (fs_contrast_times), medians over the same calls.
                The run heads (fs_passages.hip) and the host's waits make up the rest
  sweeps_all_atomics_ms
                the sweeps under FS_CONTRAST_PRECHECK=0, the same way; precheck_over_all is
                sweeps_ms over it, and `same` says the two settings wrote the same bytes
  units, active, permutations
                units; works with a passage; permutations
  product_ands_per_s
                ceil(units / 64) * 64 * ceil((permutations + 2) / 64) * 64 * ceil(active / 64)
                64-bit ANDs, what the product does with its padding, over product_ms
  pairs_count_ms, pairs_ands_per_s, product_over_pairs
                the count pass of fs_pairs_rows on the same records in the same process (existing
                code over the same tile_counts: tiles on and above the diagonal, ceil(script / 64)
                words each) and its ANDs per second counted the same way; the ratio of the two
                rates
  totals_ms, selection_over_totals
                k_int_totals of fs_intervals_rows alone (a call without units) at the same
                n_works and as many replicates: one hash per work and replicate, the floor a
                selection of three histogram passes cannot go under; selection_ms over it
  restated      the units, the permutations and their order compared with
                tests/contrast_restated.py on the records of the first --oracle-works works at
                --oracle-permutations permutations, every field
  source        the hash of the library's sources the line was measured on (_lib.source_hash)
One line per row also goes to --out (default profiles/contrast_bench.jsonl).

usage: python tools/contrast_bench.py [--records N] [--reps R] [--permutations P]
           [--shapes small,medium,large,shared] [--unit word,scene] [--shared-works W]
           [--oracle-works 400] [--oracle-permutations 64]
           [--out profiles/contrast_bench.jsonl] [--device D]
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

PASSES = ("incidence_ms", "selection_ms", "product_ms", "sweeps_ms")


def up64(x):
    return (x + 63) // 64 * 64


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast_bench.jsonl"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    from fandom_search_amd import _lib, abi, contrast, quotes, synth
    from fandom_search_amd.companions import active_works
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    from tests import contrast_restated as cn
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    L = _lib.load()
    dev = "cuda:%d" % args.device
    P = args.permutations
    out = open(args.out, "w") if args.out else None
    os.environ.pop("FS_CONTRAST_PRECHECK", None)
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        side = np.where(np.arange(n_works) < n_works // 3, 1, 2).astype(np.uint8)
        d_side = torch.from_numpy(side).to(dev)
        active = active_works(*cols, 6, 0)
        # the count pass of pairs: no room for pairs, so the call ends behind it
        p_works = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        pms, p_count = (C.c_double * 4)(), []
        for k in range(args.reps + 1):
            try:
                ix.pairs_device(d_rows.data_ptr(), n, n_works, out_ptrs=(p_works.data_ptr(), 0),
                                cap=0)
            except _lib.FsError as e:
                if e.code != abi.FS_E_CAPACITY:
                    raise
            L.fs_pairs_times(pms)
            if k:
                p_count.append(pms[1])
        a_tiles = (active + 63) // 64
        pairs_ands = a_tiles * (a_tiles + 1) // 2 * 64 * 64 * ((N_SCRIPT + 63) // 64)
        # k_int_totals alone: intervals without units
        d_reps = torch.empty(P * abi.INTERVAL_REPLICATE_DTYPE.itemsize, dtype=torch.uint8,
                             device=dev)
        none_map = torch.from_numpy(np.full(N_SCRIPT, abi.FS_NONE, dtype=np.uint32)).to(dev)
        torch_ready()
        ims, totals = (C.c_double * 6)(), []
        for k in range(args.reps + 1):
            ix.intervals_device(d_rows.data_ptr(), n, n_works, none_map.data_ptr(), 0,
                                replicates=P, out_ptrs=(0, d_reps.data_ptr()))
            L.fs_intervals_times(ims)
            if k:
                totals.append(ims[1])
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
            d_units = torch.empty(max(1, n_units) * abi.CONTRAST_UNIT_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            d_perms = torch.empty(P * abi.CONTRAST_PERM_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            torch_ready()
            ptrs = (d_units.data_ptr(), d_perms.data_ptr())
            res = {"source": _lib.source_hash(), "records": n, "shape": shape, "unit": unit,
                   "works": n_works, "units": n_units, "active": active, "permutations": P,
                   "reps": args.reps}

            def call():
                ix.contrast_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_units,
                                   d_side.data_ptr(), permutations=P, out_ptrs=ptrs)
            seen = []
            for precheck in ("1", "0"):
                os.environ["FS_CONTRAST_PRECHECK"] = precheck
                call()                                                     # warm-up
                total, passes = [], []
                for _ in range(args.reps):
                    ms = (C.c_double * 5)()
                    t = time.perf_counter()
                    call()
                    total.append((time.perf_counter() - t) * 1e3)
                    L.fs_contrast_times(ms)
                    passes.append(list(ms))
                seen.append((d_units.cpu().numpy().tobytes(), d_perms.cpu().numpy().tobytes()))
                if precheck == "1":
                    res["contrast_ms"] = round(float(np.median(total)), 3)
                    for k, name in enumerate(PASSES):
                        res[name] = round(float(np.median([p[k] for p in passes])), 3)
                else:
                    res["sweeps_all_atomics_ms"] = round(float(np.median([p[3] for p in passes])), 3)
            os.environ.pop("FS_CONTRAST_PRECHECK", None)
            res["same"] = seen[0] == seen[1]
            res["precheck_over_all"] = round(res["sweeps_ms"] / res["sweeps_all_atomics_ms"], 3) \
                if res["sweeps_all_atomics_ms"] > 0 else None
            ands = up64(n_units) * up64(P + 2) * ((active + 63) // 64)
            res["product_ands_per_s"] = float("%.3g" % (ands / (res["product_ms"] * 1e-3))) \
                if res["product_ms"] > 0 else None
            res["pairs_count_ms"] = round(float(np.median(p_count)), 3)
            res["pairs_ands_per_s"] = float("%.3g" % (pairs_ands / (res["pairs_count_ms"] * 1e-3))) \
                if res["pairs_count_ms"] > 0 else None
            res["product_over_pairs"] = round(res["product_ands_per_s"] / res["pairs_ands_per_s"], 3) \
                if res["product_ands_per_s"] and res["pairs_ands_per_s"] else None
            res["totals_ms"] = round(float(np.median(totals)), 3)
            res["selection_over_totals"] = round(res["selection_ms"] / res["totals_ms"], 3) \
                if res["totals_ms"] > 0 else None
            # the restatement on the first works
            few = min(args.oracle_works, n_works)
            keep = cols[0] < few
            sub = tuple(c[keep] for c in cols)
            t = time.perf_counter()
            want = cn.contrast(list(zip(*(c.tolist() for c in sub))), few, N_SCRIPT,
                               unit_of.tolist(), n_units, side[:few].tolist(), 6, 0, 5,
                               args.oracle_permutations, 0, 32)
            res["restated_s"] = round(time.perf_counter() - t, 3)
            got = contrast.find_contrast(*sub, few, N_SCRIPT, unit_of, n_units, side[:few], 6, 0, 5,
                                         args.oracle_permutations, 0, 32, args.device,
                                         a_counts=True)
            ok = got[2].tolist() == want[2]
            for name in cn.UNIT_KEYS:
                ok = ok and got[0][name].tolist() == [d[name] for d in want[0]]
            for name in cn.PERM_KEYS:
                ok = ok and got[1][name].tolist() == [d[name] for d in want[1]]
            res["restated"] = bool(ok)
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
