#!/usr/bin/env python3
"""`lines` timings, one JSON line per shape of the works and setting of the zero-skip:
  records       the three record mixes of tools/works_bench.py (small, medium, large) and
                `shared` of tools/pairs_bench.py over a 20 000-word script
  lines         a seeded line table: lines of 1 to 23 words (mean about 12), one in a hundred a
                monologue of 150 to 300.  It sits in HBM before the clock starts
  skip          1: the walk passes over a (line, column) whose incidence word is zero, the
                default; 0: FS_LINES_SKIP=0, every (line, column) is walked
  lines_ms      fs_lines_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --most 50
  tables_ms, walk_ms
                HIP-event times of its passes (fs_lines_times), medians over the same calls:
                coverage, incidence and the cell offsets; the walk with the per-work records.
                The run heads (fs_passages.hip) and the host's waits make up the rest of lines_ms
  n_lines, active, cells
                lines; works with a passage; cells
  companions_incidence_ms
                the incidence pass of fs_companions_rows on the same records in the same process
                with the unit map word -> line (--min-both above every count, so nothing is
                placed): the sibling pass that builds the same line x work bit matrix
  pairs_coverage_ms
                the coverage pass of fs_pairs_rows, the same way
  oracle_s      the test oracle (tests/lines_restated.py) on the same records where it is
                affordable (up to --oracle-max active works); its result is compared with the
                device's
  build         the hash of the library's sources (_lib.source_hash) the row was measured on

usage: python tools/lines_bench.py [--records N] [--reps R] [--shapes small,medium,large,shared]
           [--shared-works W] [--oracle-max A] [--device D]
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
from tools.works_bench import N_SCRIPT, records   # noqa: E402

PASSES = ("tables_ms", "walk_ms")


def line_table(seed=7):
    rng = np.random.default_rng(seed)
    at, first = 0, []
    while at < N_SCRIPT:
        first.append(at)
        at += int(rng.integers(150, 301)) if rng.random() < 0.01 else int(rng.integers(1, 24))
    return np.array(first + [N_SCRIPT], dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-max", type=int, default=600)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    import torch
    from fandom_search_amd import _lib, abi, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    words = synth.vocab_words()
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    L = _lib.load()
    dev = "cuda:%d" % args.device
    table = line_table()
    n_lines = len(table) - 1
    line_of = np.repeat(np.arange(n_lines, dtype=np.uint32), np.diff(table.astype(np.int64)))
    d_table = torch.from_numpy(table).to(dev)
    d_map = torch.from_numpy(line_of).to(dev)
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        torch_ready()
        # the two siblings beside it, once per shape: nothing kept, nothing placed
        d_pw = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cu = torch.empty(n_lines * abi.COMPANION_UNIT_DTYPE.itemsize, dtype=torch.uint8,
                           device=dev)
        d_none = torch.empty(64, dtype=torch.uint8, device=dev)
        torch_ready()
        cover, incidence = [], []
        for rep in range(args.reps + 1):
            ms = (C.c_double * 4)()
            ix.pairs_device(d_rows.data_ptr(), n, n_works, 6, 0, 1 << 30,
                            out_ptrs=(d_pw.data_ptr(), d_none.data_ptr()), cap=1)
            L.fs_pairs_times(ms)
            cover.append(ms[0])
            ix.companions_device(d_rows.data_ptr(), n, n_works, d_map.data_ptr(), n_lines, 6, 0,
                                 1 << 30, 0, out_ptrs=(d_cu.data_ptr(), d_none.data_ptr()), cap=1)
            L.fs_companions_times(ms)
            incidence.append(ms[0])
        host = None
        for skip in ("1", "0"):
            os.environ["FS_LINES_SKIP"] = skip
            got = ix.lines_device(d_rows.data_ptr(), n, n_works, d_table.data_ptr(), n_lines)  # warm-up
            if host is None:
                host = got
            else:
                assert all((a == b).all() for a, b in zip(got, host)), "FS_LINES_SKIP changes a result"
            na, nc = len(got[1]), len(got[2])
            d_lines = torch.empty(n_lines * abi.LINE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_works = torch.empty(max(1, na) * abi.LINE_WORK_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            d_cells = torch.empty(max(1, nc) * abi.LINE_CELL_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            torch_ready()
            ptrs = (d_lines.data_ptr(), d_works.data_ptr(), d_cells.data_ptr())
            total, passes = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 3)()
                t = time.perf_counter()
                ix.lines_device(d_rows.data_ptr(), n, n_works, d_table.data_ptr(), n_lines,
                                out_ptrs=ptrs, caps=(max(1, na), max(1, nc)))
                total.append((time.perf_counter() - t) * 1e3)
                L.fs_lines_times(ms)
                passes.append(list(ms))
            res = {"build": _lib.source_hash(), "records": n, "shape": shape, "skip": int(skip),
                   "works": n_works,
                   "n_lines": n_lines, "active": na, "cells": nc,
                   "lines_ms": round(float(np.median(total)), 3)}
            for k, name in enumerate(PASSES):
                res[name] = round(float(np.median([p[k] for p in passes])), 3)
            res["companions_incidence_ms"] = round(float(np.median(incidence[1:])), 3)
            res["pairs_coverage_ms"] = round(float(np.median(cover[1:])), 3)
            if skip == "1" and na <= args.oracle_max:
                from tests import lines_restated as lr
                recs = list(zip(*(c.tolist() for c in cols)))
                t = time.perf_counter()
                want = lr.lines(recs, n_works, N_SCRIPT, table.tolist(), 6, 0, 50)
                res["oracle_s"] = round(time.perf_counter() - t, 3)
                for part, keys, mine in zip(want, (lr.LINE_KEYS, lr.WORK_KEYS, lr.CELL_KEYS), host):
                    assert len(part) == len(mine)
                    for name in keys:
                        assert mine[name].tolist() == [d[name] for d in part], name
            print(json.dumps(res), flush=True)
        os.environ.pop("FS_LINES_SKIP", None)
    ix.close()


if __name__ == "__main__":
    main()
