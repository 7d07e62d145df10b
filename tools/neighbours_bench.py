#!/usr/bin/env python3
"""`neighbours` timings, one JSON line per shape of the works:
  records       N synthetic match records sorted by (work, fan_ix), the mixes of
                tools/pairs_bench.py over a 20 000-word script (small, medium, large, shared)
  neighbours_ms fs_neighbours_rows on those records already in HBM (median of --reps calls
                after a warm-up, host clock around the synchronous call), --top 10 and the
                defaults otherwise
  coverage_ms, weights_ms, product_ms, place_ms, detail_ms
                HIP-event times of its passes (fs_neighbours_times), medians over the same
                calls; the run heads (fs_passages.hip) and the host's waits make up the rest
  plain_ms, plain_product_ms
                the same call and its product pass under FS_NEIGHBOURS_MFMA=0, and
                product_ratio = plain_product_ms / product_ms
  pairs_ms, pairs_count_ms
                the yardstick: fs_pairs_rows (--min-shared 6) and its count pass on the same
                records in the same process
  active, listed, words_walked
                works with a passage; listed pairs; `words_walked`: the share of the (row
                tile, column tile, 64-bit word) triples in which both tiles have a record, about
                what the product walks (bridged words are not counted)
  oracle_s      the test oracle (tests/neighbours_restated.py) on the same records, up to
                --oracle-max active works: every field of the three arrays is compared
  source        the hash of the library's sources the line was measured on (_lib.source_hash)
One line per row also goes to --out (default profiles/neighbours_bench.jsonl).

usage: python tools/neighbours_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,shared] [--shared-works W] [--oracle-max A]
           [--out profiles/neighbours_bench.jsonl] [--device D]
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

from tools.pairs_bench import shared_records          # noqa: E402
from tools.works_bench import N_SCRIPT, records       # noqa: E402

PASSES = ("coverage_ms", "weights_ms", "product_ms", "place_ms", "detail_ms")
TOP = 10


def words_walked(cols, works):
    """The share of (row tile, column tile, word) triples the product walks: per word the
    square of the tiles with a bit in it."""
    active = np.nonzero(works["covered"])[0]
    number = np.full(len(works), -1, dtype=np.int64)
    number[active] = np.arange(len(active))
    tiles = (len(active) + 63) // 64
    nk = (N_SCRIPT + 63) // 64
    # (an upper bound of the coverage: the records' own words; bridged words lie between them)
    keep = number[cols[0]] >= 0
    cell = np.unique((number[cols[0]][keep] // 64) * nk + cols[2][keep] // 64)
    per_word = np.bincount(cell % nk, minlength=nk).astype(np.float64)
    return float((per_word ** 2).sum() / (tiles * tiles * nk)) if tiles else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--oracle-max", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours_bench.jsonl"))
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
        os.environ["FS_NEIGHBOURS_MFMA"] = "1"
        host = ix.neighbours_device(d_rows.data_ptr(), n, n_works, top=TOP)   # sizes the buffer
        cap = max(1, len(host[2]))
        d_out = [torch.empty(max(1, k) * dt.itemsize, dtype=torch.uint8, device=dev)
                 for k, dt in ((n_works, abi.NEIGHBOUR_WORK_DTYPE),
                               (N_SCRIPT, abi.NEIGHBOUR_WORD_DTYPE), (cap, abi.NEIGHBOUR_DTYPE))]
        torch_ready()
        ptrs = tuple(b.data_ptr() for b in d_out)
        active = int((host[0]["covered"] > 0).sum())
        res = {"source": _lib.source_hash(), "records": n, "shape": shape, "works": n_works,
               "active": active, "top": TOP, "reps": args.reps,
               "words_walked": float("%.3g" % words_walked(cols, host[0]))}
        for mfma, total_name, prefix in (("1", "neighbours_ms", ""), ("0", "plain_ms", "plain_")):
            os.environ["FS_NEIGHBOURS_MFMA"] = mfma
            got = ix.neighbours_device(d_rows.data_ptr(), n, n_works, top=TOP, out_ptrs=ptrs,
                                       cap=cap)                                # the warm-up
            total, passes = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 6)()
                t = time.perf_counter()
                got = ix.neighbours_device(d_rows.data_ptr(), n, n_works, top=TOP, out_ptrs=ptrs,
                                           cap=cap)
                total.append((time.perf_counter() - t) * 1e3)
                L.fs_neighbours_times(ms)
                passes.append(list(ms))
            res["listed"] = got
            res[total_name] = round(float(np.median(total)), 3)
            for k, name in enumerate(PASSES):
                if mfma == "1" or name == "product_ms":
                    res[prefix + name] = round(float(np.median([p[k] for p in passes])), 3)
            mine = tuple(b.cpu().numpy().view(dt)[:k] for b, dt, k in zip(
                d_out, (abi.NEIGHBOUR_WORK_DTYPE, abi.NEIGHBOUR_WORD_DTYPE, abi.NEIGHBOUR_DTYPE),
                (n_works, N_SCRIPT, got)))
            for a, b in zip(mine, host):                   # both products, and the first call
                assert len(a) == len(b) and (a == b).all()
        del os.environ["FS_NEIGHBOURS_MFMA"]
        res["product_ratio"] = round(res["plain_product_ms"] / res["product_ms"], 2) \
            if res["product_ms"] > 0 else None
        # the yardstick
        pw, pp = ix.pairs_device(d_rows.data_ptr(), n, n_works)
        pcap = max(1, len(pp))
        d_pw = torch.empty(max(1, n_works) * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8,
                           device=dev)
        d_pp = torch.empty(pcap * abi.PAIR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        total, count = [], []
        for _ in range(args.reps):
            ms = (C.c_double * 4)()
            t = time.perf_counter()
            ix.pairs_device(d_rows.data_ptr(), n, n_works, out_ptrs=(d_pw.data_ptr(),
                                                                     d_pp.data_ptr()), cap=pcap)
            total.append((time.perf_counter() - t) * 1e3)
            L.fs_pairs_times(ms)
            count.append(ms[1])
        res["pairs"] = len(pp)
        res["pairs_ms"] = round(float(np.median(total)), 3)
        res["pairs_count_ms"] = round(float(np.median(count)), 3)
        if active <= args.oracle_max:
            from tests import neighbours_restated as nr
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = nr.neighbours(recs, n_works, N_SCRIPT, top=TOP)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            for a, b, keys in zip(host, want, (nr.WORK_KEYS, nr.WORD_KEYS, nr.NEIGHBOUR_KEYS)):
                assert len(a) == len(b)
                for name in keys:
                    assert a[name].tolist() == [d[name] for d in b], name
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    ix.close()
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
