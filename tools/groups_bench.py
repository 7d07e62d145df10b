#!/usr/bin/env python3
"""`groups` timings, one JSON line per (shape of the works, membership):
  records       N synthetic match records sorted by (work, fan_ix), the mixes of
                tools/works_bench.py over a 20 000-word script
  shape         small: a new work every four records on average; medium: every thousand;
                large: ten works of N / 10 records
  membership    all: one group of all works; each: one group per work; tags: twenty groups per
                work out of 5 000, drawn with probability ~ 1 / rank
  groups_ms     fs_groups_rows on those records already in HBM (median of --reps calls after a
                warm-up, host clock around the synchronous call), --min-words 6 --max-gap 0
                --min-works 1, fifty scenes; the host's counting sort of the membership is
                inside it
  tables_ms, reduce_ms, offsets_ms, place_ms
                HIP-event times of its passes (fs_groups_times), medians over the same calls
  works_rows_ms fs_works_rows on the same records, for scale
  oracle_s      the test oracle (tests/groups_restated.py) on the same records where works x
                groups <= --oracle-max (its result is compared with the device's); a call the
                library refuses (FS_GROUPS_MAX_BYTES) is reported as refused

usage: python tools/groups_bench.py [--records N] [--reps R] [--shapes small,medium,large]
                                    [--memberships all,each,tags] [--oracle-max P] [--device D]
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

PASSES = ("tables_ms", "reduce_ms", "offsets_ms", "place_ms")
N_SCENES = 50
TAG_GROUPS, TAGS_PER_WORK = 5000, 20


def membership(kind, n_works, seed=2):
    """(list of group lists, n_groups)."""
    if kind == "all":
        return [[0]] * n_works, 1
    if kind == "each":
        return [[w] for w in range(n_works)], n_works
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, TAG_GROUPS + 1)
    p /= p.sum()
    return [sorted(rng.choice(TAG_GROUPS, size=TAGS_PER_WORK, replace=False, p=p).tolist())
            for _ in range(n_works)], TAG_GROUPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="small,medium,large")
    ap.add_argument("--memberships", default="all,each,tags")
    ap.add_argument("--oracle-max", type=int, default=2_000_000)
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
    label_of = (np.arange(N_SCRIPT, dtype=np.uint32) * N_SCENES // N_SCRIPT).astype(np.uint32)
    for shape in args.shapes.split(","):
        cols = records(args.records, shape)
        n = len(cols[0])
        n_works = int(cols[0][-1]) + 1
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
            rows[name] = col
        rows["comb"] = np.where(np.arange(n) % 3 == 0, 0.05, 0.0)
        d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
        torch_ready()
        ix.works_device(d_rows.data_ptr(), n, n_works, label_of, N_SCENES)      # warm-up
        t = time.perf_counter()
        ix.works_device(d_rows.data_ptr(), n, n_works, label_of, N_SCENES)
        works_ms = round((time.perf_counter() - t) * 1e3, 3)    # (with its copies to the host)
        for kind in args.memberships.split(","):
            mem, n_groups = membership(kind, n_works)
            off = np.zeros(n_works + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(m) for m in mem])
            grp = np.fromiter((g for m in mem for g in m), dtype=np.uint32, count=int(off[-1]))
            res = {"records": n, "shape": shape, "membership": kind, "works": n_works,
                   "groups": n_groups, "works_rows_ms": works_ms}
            call = dict(mem_off=off, mem_grp=grp, n_groups=n_groups, label_of=label_of,
                        n_labels=N_SCENES)
            try:
                host = ix.groups_device(d_rows.data_ptr(), n, n_works, **call)   # sizes the buffers
            except _lib.FsError as e:
                res["refused"] = str(e)
                print(json.dumps(res), flush=True)
                continue
            caps = (max(1, len(host[1])), max(1, len(host[2])))
            d_out = [torch.empty(k * dt.itemsize, dtype=torch.uint8, device=dev) for k, dt in
                     ((n_groups, abi.GROUP_DTYPE), (caps[0], abi.GROUP_CELL_DTYPE),
                      (caps[1], abi.GROUP_WORD_DTYPE))]
            torch_ready()
            ptrs = tuple(t_.data_ptr() for t_ in d_out)
            total, passes = [], []
            for _ in range(args.reps):
                ms = (C.c_double * 4)()
                t = time.perf_counter()
                got = ix.groups_device(d_rows.data_ptr(), n, n_works, out_ptrs=ptrs, caps=caps,
                                       **call)
                total.append((time.perf_counter() - t) * 1e3)
                L.fs_groups_times(ms)
                passes.append(list(ms))
            res.update(cells=got[0], word_rows=got[1],
                       groups_ms=round(float(np.median(total)), 3))
            for k, name in enumerate(PASSES):
                res[name] = round(float(np.median([p[k] for p in passes])), 3)
            if n_works * n_groups <= args.oracle_max:
                from tests import groups_restated
                exact = (rows["comb"] <= 0).tolist()
                recs = list(zip(*(c.tolist() for c in cols[:3]), exact))
                t = time.perf_counter()
                want = groups_restated.groups(recs, n_works, N_SCRIPT, mem, n_groups,
                                              label_of.tolist(), N_SCENES, 6, 0, 1)
                res["oracle_s"] = round(time.perf_counter() - t, 3)
                for part, have, keys in zip(want, host, (groups_restated.GROUP_KEYS,
                                                         groups_restated.CELL_KEYS,
                                                         groups_restated.WORD_KEYS)):
                    assert len(part) == len(have)
                    for name in keys:
                        assert have[name].tolist() == [d[name] for d in part], name
            print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
