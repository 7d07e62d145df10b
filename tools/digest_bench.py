#!/usr/bin/env python3
"""`digest` timings, one JSON line per shape of the records and round path:
  records       the three record mixes of tools/works_bench.py (small, medium, large) and `shared`
                of tools/pairs_bench.py, over a 20 000-word script
  lazy          1: a tile of 64 works is left unread in a round when the gains its works last had
                are all below the gain already found, the default; 0: FS_DIGEST_LAZY=0, every
                tile with a work left is read in every round
  digest_ms     fs_digest_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --picks 0 --cover 100 --min-gain 1
  coverage_ms, rounds_ms, works_ms, passes_ms
                HIP-event times of its passes and their total (fs_digest_times), medians over the
                same calls.  The run heads (fs_passages.hip) make up the rest
  active, picks, total_words
                works with a passage; picks made; script words any work covers
  rounds        rounds the host enqueued (a batch is enqueued whole)
  tiles, tiles_per_round
                tiles of 64 active works; tiles the gain pass read per pick (round 1 reads none),
                counted in one more call under FS_DIGEST_COUNT=1
  pairs_ms, pairs_count_ms
                fs_pairs_rows (--min-shared 6, nothing placed: a capacity of one pair) and its
                count pass on the same records in the same process, for scale (host clock; HIP
                events)
  oracle_s      the test oracle (tests/digest_restated.py) on the same records where it is
                affordable (up to --oracle-max active works), else on the records of the first
                --oracle-max works; its result is compared with the device's on the same records
  build         the hash of the library's sources (_lib.source_hash) the row was measured on

usage: python tools/digest_bench.py [--records N] [--reps R] [--shapes small,medium,large,shared]
           [--shared-works W] [--oracle-max A] [--out profiles/digest_bench.jsonl] [--device D]
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

from tools.pairs_bench import shared_records       # noqa: E402
from tools.works_bench import N_SCRIPT, records    # noqa: E402

PASSES = ("coverage_ms", "rounds_ms", "works_ms", "passes_ms")
FLAGS = (6, 0, 0, 100, 1)        # --min-words --max-gap --picks --cover --min-gain


def check_oracle(ix, cols, n_works, limit, abi, torch, dev):
    """Seconds the oracle takes on the records of the works below `limit`, compared field by
    field with the device on the same records."""
    from fandom_search_amd.engine import torch_ready
    from tests import digest_restated as dr
    keep = cols[0] < limit
    part = tuple(np.ascontiguousarray(c[keep]) for c in cols)
    n_works = min(n_works, limit)
    recs = list(zip(*(c.tolist() for c in part)))
    t = time.perf_counter()
    want = dr.digest(recs, n_works, N_SCRIPT, *FLAGS)
    took = time.perf_counter() - t
    rows = np.zeros(max(1, len(part[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), part):
        rows[name][:len(col)] = col
    d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
    torch_ready()
    got = ix.digest_device(d_rows.data_ptr(), len(part[0]), n_works, *FLAGS)
    assert got[2] == want[2]
    for mine, theirs, keys in zip(got[:2], want[:2], (dr.PICK_KEYS, dr.WORK_KEYS)):
        assert len(mine) == len(theirs)
        for name in keys:
            assert mine[name].tolist() == [d[name] for d in theirs], name
    return took, len(want[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-max", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "digest_bench.jsonl"))
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
    lines = []
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        # the sibling beside it, once per shape: nothing placed
        d_pw = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_none = torch.empty(64, dtype=torch.uint8, device=dev)
        torch_ready()
        pair_ms, count_ms = [], []
        for rep in range(args.reps + 1):
            ms = (C.c_double * 4)()
            t = time.perf_counter()
            try:
                ix.pairs_device(d_rows.data_ptr(), n, n_works, 6, 0, 6,
                                out_ptrs=(d_pw.data_ptr(), d_none.data_ptr()), cap=1)
            except _lib.FsError as e:                      # (more than one pair: not placed)
                if e.code != abi.FS_E_CAPACITY:
                    raise
            pair_ms.append((time.perf_counter() - t) * 1e3)
            L.fs_pairs_times(ms)
            count_ms.append(ms[1])
        host = None
        for lazy in ("1", "0"):
            os.environ["FS_DIGEST_LAZY"] = lazy
            got = ix.digest_device(d_rows.data_ptr(), n, n_works, *FLAGS)          # warm-up
            if host is None:
                host = got
            else:
                assert got[2] == host[2] and all((a == b).all() for a, b in zip(got[:2], host[:2])), \
                    "FS_DIGEST_LAZY changes a result"
            npk, na = len(got[0]), len(got[1])
            d_picks = torch.empty(max(1, npk) * abi.DIGEST_PICK_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            d_works = torch.empty(max(1, na) * abi.DIGEST_WORK_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            torch_ready()
            ptrs = (d_picks.data_ptr(), d_works.data_ptr())
            caps = (max(1, npk), max(1, na))
            total, passes = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 6)()
                t = time.perf_counter()
                ix.digest_device(d_rows.data_ptr(), n, n_works, *FLAGS, out_ptrs=ptrs, caps=caps)
                total.append((time.perf_counter() - t) * 1e3)
                L.fs_digest_times(ms)
                passes.append(list(ms))
            os.environ["FS_DIGEST_COUNT"] = "1"            # the tiles read, in a call of its own
            ms = (C.c_double * 6)()
            ix.digest_device(d_rows.data_ptr(), n, n_works, *FLAGS, out_ptrs=ptrs, caps=caps)
            L.fs_digest_times(ms)
            os.environ.pop("FS_DIGEST_COUNT")
            res = {"build": _lib.source_hash(), "records": n, "shape": shape, "lazy": int(lazy),
                   "works": n_works, "active": na, "picks": npk, "total_words": got[2],
                   "rounds": int(ms[4]), "tiles": (na + 63) // 64,
                   "tiles_per_round": round(ms[5] / max(1, npk), 2),
                   "digest_ms": round(float(np.median(total)), 3)}
            for k, name in enumerate(PASSES):
                res[name] = round(float(np.median([p[k] for p in passes])), 3)
            res["pairs_ms"] = round(float(np.median(pair_ms[1:])), 3)
            res["pairs_count_ms"] = round(float(np.median(count_ms[1:])), 3)
            if lazy == "1":
                res["oracle_s"], res["oracle_active"] = check_oracle(
                    ix, cols, n_works, n_works if na <= args.oracle_max else args.oracle_max,
                    abi, torch, dev)
                res["oracle_s"] = round(res["oracle_s"], 3)
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
        os.environ.pop("FS_DIGEST_LAZY", None)
    ix.close()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
