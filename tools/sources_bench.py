#!/usr/bin/env python3
"""`sources` timings over three files (K = 3), one JSON line per shape of the works:
  records       per file, the three record mixes of tools/works_bench.py (small, medium, large),
                file s drawn with seed s + 1 over the same work numbers, and `shared`: works of
                twenty passages of six words, every one of them at the same fan words in all
                three files (a stretch all scripts hold), so that every passage has two rivals
  sources_ms    fs_sources on host columns (median of --reps calls after a warm-up, host clock
                around the synchronous call: uploads, every pass and the copies back),
                --min-words 6 --max-gap 0
  passages_ms, contest_ms, union_ms, rollups_ms, total_ms
                HIP-event times of its passes (fs_sources_times), medians over the same calls
  union_all_ms, wave_contest_ms, global_contest_ms
                the union pass under FS_SOURCES_UNION=1, the contest pass under
                FS_SOURCES_PACK=0 and under FS_SOURCES_DENSE=0, the same way
  floor_ms      K calls of fs_passages on the same columns (host columns too), the same way: the
                passages alone, which the call cannot go under
  passages, rows, contests
                passages of all files; (work, script) rows; rival pairs over all pairs of files
  oracle_s      the test oracle (tests/sources_restated.py) on the same records where it takes
                a few seconds (up to --oracle-max records per file); its result is compared
                with the device's

usage: python tools/sources_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,shared] [--oracle-max N] [--device D]
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

from tools.works_bench import records   # noqa: E402

K = 3
PASSES = ("passages_ms", "contest_ms", "union_ms", "rollups_ms", "total_ms")
SWITCHES = ("FS_SOURCES_UNION", "FS_SOURCES_PACK", "FS_SOURCES_DENSE")
SHARED_WORDS, SHARED_PASSAGES, SHARED_GAP = 6, 20, 3


def shared_records(n, s):
    """n records (a multiple of six below it) of file s: passages of six words, twenty to a
    work, three fan words between two of them; the script words differ from file to file."""
    n_pass = n // SHARED_WORDS
    p = np.repeat(np.arange(n_pass, dtype=np.int64), SHARED_WORDS)
    k = np.tile(np.arange(SHARED_WORDS, dtype=np.int64), n_pass)
    work = p // SHARED_PASSAGES
    fan = (p % SHARED_PASSAGES) * (SHARED_WORDS + SHARED_GAP) + k
    orig = ((p * 7 + 100 * s) % 3000) * 6 + k
    comb = np.where((p + k + s) % 5 == 0, 0.25, 0.0)
    return work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), comb


def timed(L, call, reps):
    """Medians over reps calls after a warm-up: (host ms, [pass ms])."""
    call()
    total, passes = [], []
    for _ in range(reps):
        ms = (C.c_double * 5)()
        t = time.perf_counter()
        call()
        total.append((time.perf_counter() - t) * 1e3)
        L.fs_sources_times(ms)
        passes.append(list(ms))
    return (round(float(np.median(total)), 3),
            [round(float(np.median([p[k] for p in passes])), 3) for k in range(5)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--oracle-max", type=int, default=20_000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    from fandom_search_amd import _lib, passages, sources
    L = _lib.load()
    for name in SWITCHES:
        os.environ.pop(name, None)
    for shape in args.shapes.split(","):
        if shape == "shared":
            files = [shared_records(args.records, s) for s in range(K)]
        else:
            files = []
            for s in range(K):
                work, fan, orig, _, comb = records(args.records, shape, seed=s + 1)
                files.append((work, fan, orig, comb))
        n_works = max(int(f[0][-1]) for f in files) + 1

        def call():
            return sources.find_sources(files, n_works, 6, 0, args.device)
        found = call()
        total, passes = timed(L, call, args.reps)
        res = {"records": len(files[0][0]), "files": K, "shape": shape, "works": n_works,
               "passages": len(found[0]), "rows": len(found[1]),
               "contests": int(found[3]["contests"].sum()),
               "union_passages": int((found[0]["rival_scripts"] >= 2).sum()),
               "sources_ms": total}
        res.update(zip(PASSES, passes))
        for name, value, key, k in (("FS_SOURCES_UNION", "1", "union_all_ms", 2),
                                    ("FS_SOURCES_PACK", "0", "wave_contest_ms", 1),
                                    ("FS_SOURCES_DENSE", "0", "global_contest_ms", 1)):
            os.environ[name] = value
            forced = call()
            res[key] = timed(L, call, args.reps)[1][k]
            os.environ.pop(name)
            for a, b in zip(forced, found):
                assert (a == b).all(), name

        def floor():
            for work, fan, orig, comb in files:
                passages.find_passages(work, fan, orig, comb, comb, 6, 0, args.device)
        floor()
        times = []
        for _ in range(args.reps):
            t = time.perf_counter()
            floor()
            times.append((time.perf_counter() - t) * 1e3)
        res["floor_ms"] = round(float(np.median(times)), 3)
        if len(files[0][0]) <= args.oracle_max:
            from tests import sources_restated as sr
            recs = [list(zip(w.tolist(), f.tolist(), o.tolist(), c.tolist(), c.tolist()))
                    for w, f, o, c in files]
            t = time.perf_counter()
            want = sr.as_tuples(sr.sources(recs, 6, 0))
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            for got, tab in zip(found, want):
                assert [tuple(r) for r in got.tolist()] == tab
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
