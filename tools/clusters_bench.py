#!/usr/bin/env python3
"""`clusters` timings, one JSON line per shape of the works, `pairs` on the same records in
the same process beside it:
  records       N synthetic match records sorted by (work, fan_ix), the mixes of
                tools/works_bench.py over a 20 000-word script
  shape         small, medium, large: as tools/works_bench.py; shared: the mix of
                tools/pairs_bench.py, --shared-works works that each quote three times from the
                same twenty stretches
  clusters_ms   fs_clusters_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-shared 6 and --min-jaccard, --min-size, --common as given
  coverage_ms, links_ms, families_ms, depth_ms, merge_ms
                HIP-event times of its passes (fs_clusters_times), medians over the same calls:
                the coverage matrix; the link pass (the tile product, the links, the unions);
                roots, sizes, numbering, member lists and the per-work results; the depth pass;
                the merge pass.  The run heads (fs_passages.hip) and the host's waits make up the
                rest of clusters_ms
  pairs_ms, pairs_coverage_ms, pairs_count_ms
                fs_pairs_rows on the same records with the same --min-words, --max-gap and
                --min-shared, and its coverage and count passes (fs_pairs_times)
  active        works with a passage; families: listed families; largest: works in the largest;
                links: links in all listed families
  oracle_s      the test oracle (tests/clusters_restated.py) on the same records, up to
                --oracle-max active works (its result is compared with the device's)

usage: python tools/clusters_bench.py [--records N] [--reps R] [--shapes small,medium,large,shared]
                                      [--shared-works W] [--min-jaccard J] [--min-size Z]
                                      [--common P] [--oracle-max A] [--device D]
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

PASSES = ("coverage_ms", "links_ms", "families_ms", "depth_ms", "merge_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--min-jaccard", type=int, default=50)
    ap.add_argument("--min-size", type=int, default=2)
    ap.add_argument("--common", type=int, default=50)
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
    rule = (6, 0, 6, args.min_jaccard, args.min_size, args.common)
    for shape in args.shapes.split(","):
        cols = shared_records(args.shared_works) if shape == "shared" else \
            records(args.records, shape)[:3]
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        # the warm-up calls size the buffers
        host_works, host_found = ix.clusters_device(d_rows.data_ptr(), n, n_works, *rule)
        _, host_pairs = ix.pairs_device(d_rows.data_ptr(), n, n_works)
        cap, pcap = max(1, len(host_found)), max(1, len(host_pairs))
        d_works = torch.empty(n_works * abi.CLUSTER_WORK_DTYPE.itemsize, dtype=torch.uint8,
                              device=dev)
        d_found = torch.empty(cap * abi.CLUSTER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_pworks = torch.empty(n_works * abi.PAIR_WORK_DTYPE.itemsize, dtype=torch.uint8,
                               device=dev)
        d_pairs = torch.empty(pcap * abi.PAIR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch_ready()
        ptrs = (d_works.data_ptr(), d_found.data_ptr())
        pptrs = (d_pworks.data_ptr(), d_pairs.data_ptr())
        total, passes, ptotal, ppasses = [], [], [], []
        for _ in range(args.reps):
            ms = (C.c_double * 5)()
            t = time.perf_counter()
            got = ix.clusters_device(d_rows.data_ptr(), n, n_works, *rule, out_ptrs=ptrs, cap=cap)
            total.append((time.perf_counter() - t) * 1e3)
            L.fs_clusters_times(ms)
            passes.append(list(ms))
            pms = (C.c_double * 4)()
            t = time.perf_counter()
            ix.pairs_device(d_rows.data_ptr(), n, n_works, out_ptrs=pptrs, cap=pcap)
            ptotal.append((time.perf_counter() - t) * 1e3)
            L.fs_pairs_times(pms)
            ppasses.append(list(pms))
        active = int((host_works["covered"] > 0).sum())
        res = {"records": n, "shape": shape, "works": n_works, "active": active, "families": got,
               "largest": int(host_found["n_works"].max()) if got else 0,
               "links": int(host_found["n_links"].astype(np.int64).sum()),
               "clusters_ms": round(float(np.median(total)), 3)}
        for k, name in enumerate(PASSES):
            res[name] = round(float(np.median([p[k] for p in passes])), 3)
        res["pairs"] = len(host_pairs)
        res["pairs_ms"] = round(float(np.median(ptotal)), 3)
        res["pairs_coverage_ms"] = round(float(np.median([p[0] for p in ppasses])), 3)
        res["pairs_count_ms"] = round(float(np.median([p[1] for p in ppasses])), 3)
        if active <= args.oracle_max:
            from tests import clusters_restated
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = clusters_restated.clusters(recs, n_works, N_SCRIPT, *rule)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            got_w = d_works.cpu().numpy().view(abi.CLUSTER_WORK_DTYPE)
            got_c = d_found.cpu().numpy().view(abi.CLUSTER_DTYPE)[:got]
            assert len(want[1]) == got
            for name in clusters_restated.WORK_KEYS:
                assert got_w[name].tolist() == [d[name] for d in want[0]], name
            for name in clusters_restated.CLUSTER_KEYS:
                assert got_c[name].tolist() == [d[name] for d in want[1]], name
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
