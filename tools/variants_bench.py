#!/usr/bin/env python3
"""`ao3.py variants` timings, one JSON line per (size, mix):
  records, file_bytes, mix, spellings
                      N synthetic records written through csv.writer: passages_bench's mix of
                      works and indices, the script index folded into 2^19 words (fs_variants
                      refuses a longer script); mix "997": FAN_WORK_WORD = f<orig % 997>, the
                      reader bench's text; mix "1e5": about 10^5 spellings with a Zipf-like skew
  intern_ms           HIP-event times of fs_matches_intern(FAN_WORK_WORD): clear, insert, number,
                      copy, device_total; intern_call_ms: the host clock around the call
                      (median of --reps)
  host_dict_s         what the interning replaces: MatchFile.text over every record and a dict,
                      on the same file in the same process
  variants_ms         the host clock around fs_variants (columns already on the host)
  commands_s          `ao3.py variants` end to end under --reader device and --reader python,
                      every run a fresh process: median of --reps runs after one warm-up (python
                      reader: sizes up to --python-max, else null)

usage: python tools/variants_bench.py [--records N ...] [--mixes 997 1e5] [--reps R]
                                      [--python-max N] [--device D]
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

N_SCRIPT = 1 << 19


def write_csv(path, cols, mix, seed=3):
    work, fan, orig, dist, comb = cols
    n = len(work)
    orig = (orig % N_SCRIPT).tolist()
    if mix == "997":
        words = ("f%d" % (o % 997) for o in orig)
    else:
        rng = np.random.default_rng(seed)
        pick = (rng.random(n) ** 3 * 100_000).astype(np.int64).tolist()
        words = ("f%d" % ((o * 7 + p) % 100_003) for o, p in zip(orig, pick))
    with open(path, "w", newline="", encoding="utf-8") as fh:
        csv.writer(fh).writerows(zip(
            ("w%07d.txt" % k for k in work.tolist()), fan.tolist(), words, (1 for _ in range(n)),
            orig, ("s%d" % (o % 991) for o in orig), (2 for _ in range(n)),
            ("ANNA" for _ in range(n)), (1 for _ in range(n)), dist.tolist(),
            (3 for _ in range(n)), comb.tolist()))


def median(xs):
    return float(np.median(xs))


def command_s(path, reader, device, reps, tmp):
    times = []
    for k in range(reps + 1):                                  # the first run warms up
        t = time.perf_counter()
        subprocess.check_call([sys.executable, os.path.join(ROOT, "ao3.py"), "variants", path,
                               "-o", os.path.join(tmp, "out_%s" % reader), "--device",
                               str(device), "--reader", reader])
        times.append(time.perf_counter() - t)
    return round(median(times[1:] if reps else times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--mixes", nargs="+", default=["997", "1e5"], choices=("997", "1e5"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--python-max", type=int, default=1_000_000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from fandom_search_amd import variants
    from fandom_search_amd.matches import MatchFile
    from fandom_search_amd.passages import _FAN_WORD
    for n in args.records:
        for mix in args.mixes:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "match.csv")
                write_csv(path, records(n), mix)
                res = {"records": n, "file_bytes": os.path.getsize(path), "mix": mix}
                with MatchFile(path, args.device) as mf:
                    assert not mf.outside and mf.n == n
                    ms, calls = [], []
                    for k in range(args.reps + 1):
                        t = time.perf_counter()
                        raw, first = mf.intern(_FAN_WORD)
                        calls.append((time.perf_counter() - t) * 1e3)
                        ms.append(mf.intern_ms)
                    res["spellings"] = len(first)
                    res["intern_ms"] = {k: round(median([m[k] for m in ms[1:]]), 3) for k in ms[0]}
                    res["intern_call_ms"] = round(median(calls[1:]), 2)
                    t = time.perf_counter()
                    ids = {}
                    host = [ids.setdefault(w, len(ids)) for w in mf.text(_FAN_WORD, np.arange(n))]
                    res["host_dict_s"] = round(time.perf_counter() - t, 3)
                    assert np.array_equal(np.asarray(host, dtype=np.uint32), raw)
                    del host, ids
                    times = []
                    for k in range(args.reps + 1):
                        t = time.perf_counter()
                        words, cells = variants.find_variants(mf.work, mf.orig, raw, len(mf.names),
                                                              int(mf.orig.max()) + 1, len(first),
                                                              args.device)
                        times.append((time.perf_counter() - t) * 1e3)
                    res["cells"] = len(cells)
                    res["variants_ms"] = round(median(times[1:]), 2)
                res["commands_s"] = {"device": command_s(path, "device", args.device, args.reps, tmp)}
                res["commands_s"]["python"] = \
                    command_s(path, "python", args.device, 1, tmp) if n <= args.python_max else None
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
