#!/usr/bin/env python3
"""`pairs` timings, one JSON line per shape of the works:
  records       N synthetic match records sorted by (work, fan_ix), the mixes of
                tools/works_bench.py over a 20 000-word script
  shape         small: a new work every four records on average; medium: every thousand;
                large: ten works of N / 10 records; shared: --shared-works works that each
                quote three times from the same twenty stretches of thirty words, dense in
                pairs and sparse in coverage (its records are as many as that takes)
  pairs_ms      fs_pairs_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-shared 6
  coverage_ms, count_ms, place_ms, detail_ms
                HIP-event times of its passes (fs_pairs_times), medians over the same calls:
                the coverage matrix; the count pass with its scan and the per-work results;
                the place pass; the detail pass.  The run heads (fs_passages.hip) and the
                host's waits make up the rest of pairs_ms
  active        works with a passage; pairs: pairs kept
  word_ands_per_s   active * (active - 1) / 2 * ceil(script / 64) 64-bit ANDs, what the count
                pass owes, over count_ms
  oracle_s      the test oracle (tests/pairs_restated.py) on the same records, up to
                --oracle-max active works (its result is compared with the device's)

usage: python tools/pairs_bench.py [--records N] [--reps R] [--shapes small,medium,large,shared]
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

from tools.works_bench import N_SCRIPT, records   # noqa: E402

PASSES = ("coverage_ms", "count_ms", "place_ms", "detail_ms")


def shared_records(n_works, seed=1):
    """Works of three passages of 8..20 words, each inside one of twenty hot stretches."""
    rng = np.random.default_rng(seed)
    hot = rng.integers(0, N_SCRIPT - 30, size=20)
    work, fan, orig = [], [], []
    for w in range(n_works):
        f = 0
        for _ in range(3):
            k = int(rng.integers(8, 21))
            o0 = int(hot[rng.integers(0, 20)]) + int(rng.integers(0, 31 - k))
            work.append(np.full(k, w))
            fan.append(np.arange(f, f + k))
            orig.append(np.arange(o0, o0 + k))
            f += k + 50
    return tuple(np.concatenate(c).astype(np.uint32) for c in (work, fan, orig))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-max", type=int, default=1500)
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
    nk = (N_SCRIPT + 63) // 64
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        host_works, host_pairs = ix.pairs_device(d_rows.data_ptr(), n, n_works)   # sizes the buffer
        cap = max(1, len(host_pairs))
        d_works = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pairs = torch.empty(cap * abi.PAIR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        ptrs = (d_works.data_ptr(), d_pairs.data_ptr())
        total, passes = [], []
        for _ in range(args.reps):
            ms = (C.c_double * 4)()
            t = time.perf_counter()
            got = ix.pairs_device(d_rows.data_ptr(), n, n_works, out_ptrs=ptrs, cap=cap)
            total.append((time.perf_counter() - t) * 1e3)
            L.fs_pairs_times(ms)
            passes.append(list(ms))
        active = int((host_works["covered"] > 0).sum())
        res = {"records": n, "shape": shape, "works": n_works, "active": active, "pairs": got,
               "pairs_ms": round(float(np.median(total)), 3)}
        for k, name in enumerate(PASSES):
            res[name] = round(float(np.median([p[k] for p in passes])), 3)
        ands = active * (active - 1) // 2 * nk
        res["word_ands_per_s"] = float("%.3g" % (ands / (res["count_ms"] * 1e-3))) \
            if res["count_ms"] > 0 else None
        if active <= args.oracle_max:
            from tests import pairs_restated
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = pairs_restated.pairs(recs, n_works, N_SCRIPT, 6, 0, 6)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            got_w = d_works.cpu().numpy().view(abi.PAIR_WORK_DTYPE)
            got_p = d_pairs.cpu().numpy().view(abi.PAIR_DTYPE)[:got]
            assert len(want[1]) == got
            for name in pairs_restated.WORK_KEYS:
                assert got_w[name].tolist() == [d[name] for d in want[0]], name
            for name in pairs_restated.PAIR_KEYS:
                assert got_p[name].tolist() == [d[name] for d in want[1]], name
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
