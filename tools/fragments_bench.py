#!/usr/bin/env python3
"""`fragments` timings, one JSON line per shape of the records and spread path:
  records       the three record mixes of tools/works_bench.py (small, medium, large), `shared`
                of tools/pairs_bench.py and `lines` of tools/matrix_bench.py (31 250 works on
                five eight-word lines: every run hits one of five cells of each table), over a
                20 000-word script
  dedup         1: the runs are reduced to the distinct (first, last) before they are spread,
                the default; 0: FS_FRAGMENTS_DEDUP=0, every run is spread by itself
  fragments_ms  fs_fragments_rows on those records already in HBM (median of --reps calls after
                a warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-works 2 --min-length 3 --max-words 128
  runs_ms, spread_ms, list_ms, works_ms
                HIP-event times of its passes (fs_fragments_times), medians over the same calls.
                The run heads (fs_passages.hip) and the host's waits make up the rest
  active, fragments
                works with a passage; fragments listed
  quotes_ms     fs_quotes_rows on the same records in the same process (host clock, median)
  pairs_coverage_ms
                the coverage pass of fs_pairs_rows, the same way (HIP events; nothing placed)
  oracle_s      the test oracle (tests/fragments_restated.py) on the same records where it is
                affordable (up to --oracle-max active works); its result is compared with the
                device's
  build         the hash of the library's sources (_lib.source_hash) the row was measured on

usage: python tools/fragments_bench.py [--records N] [--reps R]
           [--shapes small,medium,large,shared,lines] [--shared-works W] [--oracle-max A]
           [--device D]
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

from tools.matrix_bench import records as matrix_records   # noqa: E402
from tools.pairs_bench import shared_records                # noqa: E402
from tools.works_bench import N_SCRIPT                      # noqa: E402

PASSES = ("runs_ms", "spread_ms", "list_ms", "works_ms")
FLAGS = (6, 0, 2, 3, 128)        # --min-words --max-gap --min-works --min-length --max-words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared,lines")
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
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            matrix_records(args.records, shape)
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        # the two siblings beside it, once per shape: nothing kept, nothing placed
        d_pw = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_qw = torch.empty(N_SCRIPT * abi.QUOTE_WORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_qr = torch.empty(N_SCRIPT * abi.QUOTE_REGION_DTYPE.itemsize, dtype=torch.uint8,
                           device=dev)
        d_none = torch.empty(64, dtype=torch.uint8, device=dev)
        torch_ready()
        cover, quote = [], []
        for rep in range(args.reps + 1):
            ms = (C.c_double * 4)()
            ix.pairs_device(d_rows.data_ptr(), n, n_works, 6, 0, 1 << 30,
                            out_ptrs=(d_pw.data_ptr(), d_none.data_ptr()), cap=1)
            L.fs_pairs_times(ms)
            cover.append(ms[0])
            t = time.perf_counter()
            ix.quotes_device(d_rows.data_ptr(), n, n_works, 6, 0, 2,
                             out_ptrs=(d_qw.data_ptr(), d_qr.data_ptr()), cap=N_SCRIPT)
            quote.append((time.perf_counter() - t) * 1e3)
        host = None
        for dedup in ("1", "0"):
            os.environ["FS_FRAGMENTS_DEDUP"] = dedup
            got = ix.fragments_device(d_rows.data_ptr(), n, n_works, *FLAGS)       # warm-up
            if host is None:
                host = got
            else:
                assert all((a == b).all() for a, b in zip(got, host)), \
                    "FS_FRAGMENTS_DEDUP changes a result"
            nf, na = len(got[0]), len(got[1])
            d_frags = torch.empty(max(1, nf) * abi.FRAGMENT_DTYPE.itemsize, dtype=torch.uint8,
                                  device=dev)
            d_works = torch.empty(max(1, na) * abi.FRAGMENT_WORK_DTYPE.itemsize,
                                  dtype=torch.uint8, device=dev)
            torch_ready()
            ptrs = (d_frags.data_ptr(), d_works.data_ptr())
            total, passes = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 5)()
                t = time.perf_counter()
                ix.fragments_device(d_rows.data_ptr(), n, n_works, *FLAGS, out_ptrs=ptrs,
                                    caps=(max(1, nf), max(1, na)))
                total.append((time.perf_counter() - t) * 1e3)
                L.fs_fragments_times(ms)
                passes.append(list(ms))
            res = {"build": _lib.source_hash(), "records": n, "shape": shape,
                   "dedup": int(dedup), "works": n_works, "active": na, "fragments": nf,
                   "fragments_ms": round(float(np.median(total)), 3)}
            for k, name in enumerate(PASSES):
                res[name] = round(float(np.median([p[k] for p in passes])), 3)
            res["quotes_ms"] = round(float(np.median(quote[1:])), 3)
            res["pairs_coverage_ms"] = round(float(np.median(cover[1:])), 3)
            if dedup == "1" and na <= args.oracle_max:
                from tests import fragments_restated as fr
                recs = list(zip(*(c.tolist() for c in cols)))
                t = time.perf_counter()
                want = fr.fragments(recs, n_works, N_SCRIPT, *FLAGS)
                res["oracle_s"] = round(time.perf_counter() - t, 3)
                for part, keys, mine in zip(want, (fr.FRAGMENT_KEYS, fr.WORK_KEYS), host):
                    assert len(part) == len(mine)
                    for name in keys:
                        assert mine[name].tolist() == [d[name] for d in part], name
            print(json.dumps(res), flush=True)
        os.environ.pop("FS_FRAGMENTS_DEDUP", None)
    ix.close()


if __name__ == "__main__":
    main()
