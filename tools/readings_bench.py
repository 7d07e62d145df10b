#!/usr/bin/env python3
"""`ao3.py readings` timings, one JSON line per (size, mix):
  records, file_bytes, mix, spellings
                      N synthetic records written through csv.writer, the files of
                      variants_bench: mix "997": FAN_WORK_WORD = f<orig % 997>; mix "1e5": about
                      10^5 spellings with a Zipf-like skew
  passages, spans, readings
                      what fs_readings finds under --min-words 6 --max-gap 0
  readings_ms         HIP-event times of fs_readings and its passes (fs_readings_times): passages,
                      tables, spans, readings, copy_out, total; readings_call_ms: the host clock
                      around the call (columns already on the host).  Medians of --reps calls
                      after a warm-up
  passages_call_ms, variants_call_ms
                      the host clock around fs_passages and fs_variants on the same records in
                      the same process, the same medians
  oracle_s            tests/readings_restated.py on the same records (sizes up to --oracle-max,
                      else null)
  commands_s          `ao3.py readings` end to end under --reader device and --reader python,
                      every run a fresh process under its own time limit: median of --command-reps
                      runs after one warm-up (python reader: one run, sizes up to --python-max,
                      else null)

usage: python tools/readings_bench.py [--records N ...] [--mixes 997 1e5] [--reps R]
                                      [--command-reps R] [--python-max N] [--oracle-max N]
                                      [--device D]
"""

import argparse
import ctypes as C
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
from tools.variants_bench import write_csv    # noqa: E402

COMMAND_LIMIT_S = 900


def median(xs):
    return float(np.median(xs))


def command_s(path, reader, device, reps, tmp):
    times = []
    for k in range(reps + 1):                                  # the first run warms up
        t = time.perf_counter()
        subprocess.check_call(["timeout", "-k", "10", str(COMMAND_LIMIT_S), sys.executable,
                               os.path.join(ROOT, "ao3.py"), "readings", path, "-o",
                               os.path.join(tmp, "out_%s" % reader), "--device", str(device),
                               "--reader", reader])
        times.append(time.perf_counter() - t)
    return round(median(times[1:] if reps else times), 3)


def timed(reps, call):
    """(median ms of `reps` calls after a warm-up, the last result)."""
    times, out = [], None
    for k in range(reps + 1):
        t = time.perf_counter()
        out = call()
        times.append((time.perf_counter() - t) * 1e3)
    return round(median(times[1:]), 2), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--mixes", nargs="+", default=["997", "1e5"], choices=("997", "1e5"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--command-reps", type=int, default=3)
    ap.add_argument("--python-max", type=int, default=1_000_000)
    ap.add_argument("--oracle-max", type=int, default=1_000_000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from fandom_search_amd import _lib, abi, passages, readings, variants
    from fandom_search_amd.matches import MatchFile
    from fandom_search_amd.passages import _FAN_WORD
    L = _lib.load()
    for n in args.records:
        for mix in args.mixes:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "match.csv")
                write_csv(path, records(n), mix)
                res = {"records": n, "file_bytes": os.path.getsize(path), "mix": mix}
                with MatchFile(path, args.device) as mf:
                    assert not mf.outside and mf.n == n
                    raw, first = mf.intern(_FAN_WORD)
                    order, work, fan, orig, dist, comb = mf.sorted()
                    spell = raw[order]
                    n_works, n_script = len(mf.names), int(orig.max()) + 1
                res["spellings"] = len(first)
                passes = []

                def call():
                    out = readings.find_readings(work, fan, orig, spell, n_works, n_script,
                                                 len(first), 6, 0, args.device)
                    ms = (C.c_double * 6)()
                    L.fs_readings_times(ms)
                    passes.append(list(ms))
                    return out
                res["readings_call_ms"], (found, spans, n_pass) = timed(args.reps, call)
                res["passages"], res["spans"], res["readings"] = n_pass, len(spans), len(found)
                res["readings_ms"] = {k: round(median([p[j] for p in passes[1:]]), 3)
                                      for j, k in enumerate(abi.READINGS_MS_NAMES)}
                res["passages_call_ms"], kept = timed(args.reps, lambda: passages.find_passages(
                    work, fan, orig, dist, comb, 6, 0, args.device))
                assert len(kept) == n_pass
                res["variants_call_ms"], _ = timed(args.reps, lambda: variants.find_variants(
                    work, orig, spell, n_works, n_script, len(first), args.device))
                res["oracle_s"] = None
                if n <= args.oracle_max:
                    from tests import readings_restated as rr
                    recs = list(zip(work.tolist(), fan.tolist(), orig.tolist(), spell.tolist()))
                    t = time.perf_counter()
                    want = rr.readings(recs, n_works, n_script, len(first), 6, 0)
                    res["oracle_s"] = round(time.perf_counter() - t, 3)
                    assert (len(want[0]), len(want[1]), want[2]) == (len(found), len(spans), n_pass)
                    del recs, want
                res["commands_s"] = {"device": command_s(path, "device", args.device,
                                                         args.command_reps, tmp)}
                res["commands_s"]["python"] = \
                    command_s(path, "python", args.device, 0, tmp) if n <= args.python_max else None
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
