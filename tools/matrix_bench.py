#!/usr/bin/env python3
"""`matrix` timings, one JSON line per row.

Per shape of the records (row "rows"):
  records      N synthetic match records sorted by (work, fan_ix) over a 20 000-word script
  shape        small, medium, large: the mixes of tools/works_bench.py (a new work every four
               records on average; every thousand; ten works of N / 10 records); lines: a new
               work every 32 records, each quoting four of the same five eight-word lines
  matrix_ms    fs_matrix_rows on those records already in HBM (median of --reps calls after a
               warm-up, host clock around the synchronous call), -n 6
  pass_ms      the HIP-event times of the last of those calls, by pass (fs_matrix_times)
  passages_ms  fs_passages_rows on the same records, the same way
  oracle_s     the test oracle (tests/matrix_restated.py) on the same records, up to
               --oracle-max records; its counter, spans and n-grams are compared with the device's
  spans, kept  what was found

The command (row "command"), on a match CSV of the --command-shape records with its header row:
  device_s     `python ao3.py matrix --engine device --cells`, a fresh process each, median of
               --command-reps
  python_s     `python ao3.py matrix --engine python --cells`, a fresh process, run once
  same         both wrote the same bytes, dense and cells

usage: python tools/matrix_bench.py [--records N] [--reps R] [--shapes small,medium,large,lines]
           [--oracle-max N] [--command-shape medium|none] [--command-reps R] [--device D]
"""

import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from works_bench import N_SCRIPT, median_ms, records as mixed_records  # noqa: E402

NGRAM = 6
FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'FAN_WORK_WORD', 'FAN_WORK_ORTH_ID',
          'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_ORTH_ID',
          'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'BEST_MATCH_DISTANCE',
          'BEST_LEVENSHTEIN_DISTANCE', 'BEST_COMBINED_DISTANCE']


def records(n, shape, seed=1):
    if shape != "lines":
        return mixed_records(n, shape, seed)[:3]
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.int64)
    work, at = k // 32, k % 32
    line = rng.integers(0, 5, size=(n + 7) // 8)[k // 8]           # one of five famous lines
    fan = at + at // 8 * 3 + 100                                  # the four quotes lie apart
    orig = 1000 + 700 * line + at % 8
    return work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32)


def write_csv(path, cols):
    work, fan, orig = cols
    with open(path, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh)
        w.writerow(FIELDS)
        for k in range(len(work)):
            o = int(orig[k])
            w.writerow(["w%07d.txt" % work[k], int(fan[k]), "f%d" % (o % 997), 1, o,
                        "S%d" % o, 2, "ANNA", 1, 0.0, 3, 0.0])


def command(path, prefix, engine, device):
    t = time.perf_counter()
    subprocess.check_call([sys.executable, os.path.join(ROOT, "ao3.py"), "matrix", path, prefix,
                           "-n", str(NGRAM), "--cells", "--engine", engine,
                           "--device", str(device)])
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,lines")
    ap.add_argument("--oracle-max", type=int, default=1_000_000)
    ap.add_argument("--command-shape", default="medium")
    ap.add_argument("--command-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    n = args.records

    import ctypes as C

    import torch
    from fandom_search_amd import _lib, abi, matrix, synth
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    words = synth.vocab_words()
    script = synth.script_tokens(2000)
    ix = ScriptIndex(script, [words[int(t)] for t in script], synth.embedding(), synth.lsh_normals(6),
                     cfg=abi.make_config(device=args.device))
    dev = "cuda:%d" % args.device
    for shape in [s for s in args.shapes.split(",") if s]:
        cols = records(n, shape)
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        cap = n // NGRAM + 1
        d_starts = torch.empty(N_SCRIPT * 4, dtype=torch.uint8, device=dev)
        d_found = torch.empty(cap * abi.MATRIX_NGRAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pass = torch.empty(cap * abi.PASSAGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        ptrs = (d_starts.data_ptr(), d_found.data_ptr())
        found = []
        matrix_ms = median_ms(lambda: found.append(ix.matrix_device(
            d_rows.data_ptr(), n, n_works, N_SCRIPT, NGRAM, out_ptrs=ptrs, cap=cap)), args.reps)
        ms = (C.c_double * 6)()
        _lib.check(_lib.load().fs_matrix_times(ms), "fs_matrix_times")
        passages_ms = median_ms(lambda: ix.passages_device(
            d_rows.data_ptr(), n, NGRAM, 0, out_ptr=d_pass.data_ptr(), cap=cap), args.reps)
        spans, kept = found[-1]
        res = {"row": "rows", "records": n, "shape": shape, "works": n_works, "spans": spans,
               "kept": kept, "reps": args.reps, "matrix_ms": matrix_ms,
               "pass_ms": {k: round(v, 3) for k, v in zip(abi.MATRIX_MS_NAMES, ms)},
               "passages_ms": passages_ms}
        if n <= args.oracle_max:
            from tests import matrix_restated
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = matrix_restated.matrix(recs, NGRAM, N_SCRIPT)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            got = d_found.cpu().numpy().view(abi.MATRIX_NGRAM_DTYPE)[:kept]
            assert len(want[0]) == spans and got.tolist() == want[2]
            assert d_starts.cpu().numpy().view(np.uint32).tolist() == want[1]
            res["oracle"] = "equal"
        print(json.dumps(res), flush=True)
    ix.close()

    if args.command_shape and args.command_shape != "none":
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "match.csv")
            write_csv(path, records(n, args.command_shape))
            outs = {}
            device_s = []
            for k in range(args.command_reps):
                device_s.append(command(path, os.path.join(tmp, "device"), "device", args.device))
            python_s = command(path, os.path.join(tmp, "python"), "python", args.device)
            for engine in ("device", "python"):
                prefix = os.path.join(tmp, engine)
                outs[engine] = [open(f(prefix, NGRAM), "rb").read()
                                for f in (matrix.matrix_filename, matrix.cells_filename)]
            took = matrix.device_tables(path, NGRAM, args.device) is not None
            print(json.dumps({"row": "command", "records": n, "shape": args.command_shape,
                              "device_s": round(float(np.median(device_s)), 3),
                              "device_runs": args.command_reps, "python_s": round(python_s, 3),
                              "python_runs": 1, "device_engine_took_the_file": took,
                              "same": outs["device"] == outs["python"],
                              "dense_bytes": len(outs["python"][0]),
                              "cells_bytes": len(outs["python"][1])}), flush=True)


if __name__ == "__main__":
    main()
