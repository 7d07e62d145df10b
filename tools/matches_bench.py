#!/usr/bin/env python3
"""The match CSV reader's timings, one JSON line per size:
  records, file_bytes   N synthetic records (passages_bench's mix) written through csv.writer
  device_ms             HIP-event times of one fs_matches_open: upload, parity, classify, place,
                        header, rows, device_total (median of --reps)
  open_ms, read_ms      host clock around fs_matches_open and fs_matches_read
  matchfile_s           MatchFile end to end: read the file, the two calls, work numbering, order
  matchfile_parts_s     its own breakdown: read, device, host
  python_s              passages.read_matches + sort_records on the same file (sizes up to
                        --python-max)
  commands_s            `ao3.py passages / works / quotes` end to end under --reader device and
                        --reader python, every run a fresh process: median of --reps runs after
                        one warm-up (python reader: --python-reps, sizes up to --python-max)

usage: python tools/matches_bench.py [--records N ...] [--reps R] [--python-reps P]
                                     [--python-max N] [--stage {0,1}] [--device D]
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

from tools.passages_bench import records      # noqa: E402


def write_csv(path, cols):
    work, fan, orig, dist, comb = cols
    n = len(work)
    with open(path, "w", newline="", encoding="utf-8") as fh:
        orig = orig.tolist()
        csv.writer(fh).writerows(zip(
            ("w%07d.txt" % k for k in work.tolist()), fan.tolist(),
            ("f%d" % (o % 997) for o in orig), (1 for _ in range(n)), orig,
            ("s%d" % (o % 991) for o in orig), (2 for _ in range(n)), ("ANNA" for _ in range(n)),
            (1 for _ in range(n)), dist.tolist(), (3 for _ in range(n)), comb.tolist()))


def median(xs):
    return float(np.median(xs))


def command_s(cmd, path, reader, device, reps, tmp):
    times = []
    for k in range(reps + 1):                                  # the first run warms up
        t = time.perf_counter()
        subprocess.check_call([sys.executable, os.path.join(ROOT, "ao3.py"), cmd, path, "-o",
                               os.path.join(tmp, "out_%s_%s" % (cmd, reader)), "--device",
                               str(device), "--reader", reader])
        times.append(time.perf_counter() - t)
    return round(median(times[1:] if reps else times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--python-reps", type=int, default=None)
    ap.add_argument("--python-max", type=int, default=1_000_000)
    ap.add_argument("--stage", choices=("0", "1"), default=None,
                    help="FS_MATCHES_STAGE: 1 a wave stages its rows in LDS, 0 lanes read global memory")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.stage is not None:
        os.environ["FS_MATCHES_STAGE"] = args.stage
    preps = args.reps if args.python_reps is None else args.python_reps
    import ctypes as C
    from fandom_search_amd import _lib, abi, passages
    from fandom_search_amd.matches import MatchFile
    L = _lib.load()
    for n in args.records:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "match.csv")
            write_csv(path, records(n))
            res = {"records": n, "file_bytes": os.path.getsize(path),
                   "stage": os.environ.get("FS_MATCHES_STAGE", "1")}
            data = np.fromfile(path, dtype=np.uint8)
            dev, opens, reads = [], [], []
            for k in range(args.reps + 1):
                info, h = abi.FsMatchesInfo(), C.c_void_p()
                t = time.perf_counter()
                _lib.check(L.fs_matches_open(args.device, data.ctypes.data_as(C.c_void_p), len(data),
                                             C.byref(h), C.byref(info)), "fs_matches_open")
                t1 = time.perf_counter()
                assert info.status == abi.FS_MATCHES_PARSED and info.n_rows == n
                cols = [np.empty(n, dtype=d) for d in (np.uint32,) * 3 + (np.float64,) * 2]
                ix = np.empty(n, dtype=abi.MATCH_IX_DTYPE)
                t2 = time.perf_counter()
                types = L.fs_matches_read.argtypes[1:6]
                _lib.check(L.fs_matches_read(h, *(c.ctypes.data_as(t) for c, t in zip(cols, types)),
                                             ix.ctypes.data_as(C.c_void_p), n, None, 0), "fs_matches_read")
                t3 = time.perf_counter()
                L.fs_matches_close(h)
                if k:
                    dev.append(list(info.ms)[:7])
                    opens.append((t1 - t) * 1e3)
                    reads.append((t3 - t2) * 1e3)
            res["device_ms"] = {name: round(median([d[j] for d in dev]), 3)
                                for j, name in enumerate(abi.MATCHES_MS_NAMES)}
            res["open_ms"], res["read_ms"] = round(median(opens), 2), round(median(reads), 2)
            del data, cols, ix
            whole, parts = [], []
            for k in range(args.reps + 1):
                t = time.perf_counter()
                with MatchFile(path, args.device) as mf:
                    mf.order()
                    whole.append(time.perf_counter() - t)
                    parts.append(mf.times)
            res["matchfile_s"] = round(median(whole[1:]), 3)
            res["matchfile_parts_s"] = {k: round(median([p[k] for p in parts[1:]]), 3) for k in parts[0]}
            if n <= args.python_max:
                t = time.perf_counter()
                passages.sort_records(passages.read_matches(path))
                res["python_s"] = round(time.perf_counter() - t, 3)
            else:
                res["python_s"] = None
            res["commands_s"] = {}
            for cmd in ("passages", "works", "quotes"):
                res["commands_s"][cmd] = {"device": command_s(cmd, path, "device", args.device, args.reps, tmp)}
                res["commands_s"][cmd]["python"] = \
                    command_s(cmd, path, "python", args.device, preps, tmp) if n <= args.python_max else None
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
