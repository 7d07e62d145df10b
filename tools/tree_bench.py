#!/usr/bin/env python3
"""`tree` timings, one JSON line per shape of the works, `clusters` at `--min-jaccard 0 --min-size
1` on the same records in the same process beside it:
  records       N synthetic match records sorted by (work, fan_ix), the mixes of
                tools/works_bench.py over a 20 000-word script
  shape         small, medium, large: as tools/works_bench.py; shared: the mix of
                tools/pairs_bench.py, --shared-works works that each quote three times from the
                same twenty stretches
  tree_ms       fs_tree_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-shared 6 --min-level 0 and --measure as given
  cover_ms, flatten_ms, best_ms, choose_ms, hook_ms, detail_ms, replay_ms, total_ms
                its passes (fs_tree_times), medians over the same calls: HIP-event times of the
                coverage matrix, of the four passes of a round summed over the rounds and of the
                detail pass; host times of the replay and of the call inside the library
  rounds        the hooking rounds, those that added an edge; best_passes: the rounds run, one
                more when the forest is not one tree, since only a round without an edge shows
                that; one_best_ms = best_ms / best_passes
  clusters_ms, clusters_links_ms
                fs_clusters_rows on the same records with the same --min-words, --max-gap and
                --min-shared at --min-jaccard 0 --min-size 1, and its link pass
                (fs_clusters_times): the same product once, with the unions where the links are
                found.  best_over_links = one_best_ms / clusters_links_ms
  active        works with a passage; merges; levels; trees; largest: works of the largest tree
  oracle_s      the test oracle (tests/tree_restated.py) on the same records, up to --oracle-max
                active works (its result is compared with the device's, every field)
  sources       the hash of the library's sources the line was measured on

usage: python tools/tree_bench.py [--records N] [--reps R] [--shapes small,medium,large,shared]
                                  [--shared-works W] [--measure jaccard|shared] [--oracle-max A]
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

from tools.pairs_bench import shared_records      # noqa: E402
from tools.works_bench import N_SCRIPT, records   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large,shared")
    ap.add_argument("--shared-works", type=int, default=4000)
    ap.add_argument("--measure", default="jaccard", choices=("jaccard", "shared"))
    ap.add_argument("--oracle-max", type=int, default=1000)
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
    rule = (6, 0, args.measure, 6, 0)
    crule = (6, 0, 6, 0, 1, 50)
    names = abi.TREE_MS_NAMES
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
        host_works, host_merges, host_levels = ix.tree_device(d_rows.data_ptr(), n, n_works, *rule)
        _, host_found = ix.clusters_device(d_rows.data_ptr(), n, n_works, *crule)
        caps = (max(1, len(host_merges)), max(1, len(host_levels)))
        ccap = max(1, len(host_found))

        def room(count, dtype):
            return torch.empty(count * dtype.itemsize, dtype=torch.uint8, device=dev)
        d_works = room(max(1, n_works), abi.TREE_WORK_DTYPE)
        d_merges = room(caps[0], abi.TREE_MERGE_DTYPE)
        d_levels = room(caps[1], abi.TREE_LEVEL_DTYPE)
        d_cworks = room(max(1, n_works), abi.CLUSTER_WORK_DTYPE)
        d_found = room(ccap, abi.CLUSTER_DTYPE)
        torch_ready()
        ptrs = (d_works.data_ptr(), d_merges.data_ptr(), d_levels.data_ptr())
        cptrs = (d_cworks.data_ptr(), d_found.data_ptr())
        total, passes, ctotal, cpasses = [], [], [], []
        for _ in range(args.reps):
            ms = (C.c_double * len(names))()
            t = time.perf_counter()
            got = ix.tree_device(d_rows.data_ptr(), n, n_works, *rule, out_ptrs=ptrs, caps=caps)
            total.append((time.perf_counter() - t) * 1e3)
            L.fs_tree_times(ms)
            passes.append(list(ms))
            cms = (C.c_double * 5)()
            t = time.perf_counter()
            ix.clusters_device(d_rows.data_ptr(), n, n_works, *crule, out_ptrs=cptrs, cap=ccap)
            ctotal.append((time.perf_counter() - t) * 1e3)
            L.fs_clusters_times(cms)
            cpasses.append(list(cms))
        active = int((host_works["covered"] > 0).sum())
        rounds = int(passes[0][names.index("rounds")])
        best_passes = rounds + (1 if active > 1 and got[0] < active - 1 else 0)
        res = {"records": n, "shape": shape, "measure": args.measure, "works": n_works,
               "active": active, "merges": got[0], "levels": got[1],
               "trees": active - got[0],
               "largest": int(host_works["tree_works"].max()) if n_works else 0,
               "rounds": rounds, "best_passes": best_passes,
               "tree_ms": round(float(np.median(total)), 3)}
        for k, name in enumerate(names[:-1]):
            res[name + "_ms"] = round(float(np.median([p[k] for p in passes])), 3)
        res["one_best_ms"] = round(res["best_ms"] / best_passes, 3) if best_passes else 0.0
        res["clusters_ms"] = round(float(np.median(ctotal)), 3)
        res["clusters_links_ms"] = round(float(np.median([p[1] for p in cpasses])), 3)
        if best_passes and res["clusters_links_ms"]:
            res["best_over_links"] = round(res["one_best_ms"] / res["clusters_links_ms"], 2)
        if active <= args.oracle_max:
            from tests import tree_restated
            recs = list(zip(*(c.tolist() for c in cols)))
            t = time.perf_counter()
            want = tree_restated.tree(recs, n_works, N_SCRIPT, *rule)
            res["oracle_s"] = round(time.perf_counter() - t, 3)
            found = (d_works.cpu().numpy().view(abi.TREE_WORK_DTYPE),
                     d_merges.cpu().numpy().view(abi.TREE_MERGE_DTYPE)[:got[0]],
                     d_levels.cpu().numpy().view(abi.TREE_LEVEL_DTYPE)[:got[1]])
            for have, rows_, keys in zip(found, want, (tree_restated.WORK_KEYS,
                                                       tree_restated.MERGE_KEYS,
                                                       tree_restated.LEVEL_KEYS)):
                assert len(have) == len(rows_)
                for name in keys:
                    assert have[name].tolist() == [d[name] for d in rows_], name
        res["sources"] = _lib.source_hash()
        print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
