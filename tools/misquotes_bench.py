#!/usr/bin/env python3
"""`misquotes` timings, one JSON line per mix of works:
  copied    the 4 000 works of the `shared` mix of tools/pairs_bench.py; families of 2 to 50
            consecutive works carry 1 to 5 planted misquotes each (at a script word of the
            family's first work, in every member that has a record there), and 2 % of the
            records are one-off typos
  meme      the `small` mix of tools/works_bench.py (--records of them); --meme-works of its
            active works get one more passage with the same wrong word in it, and as many
            others the same passage verbatim, so that the misquote is telling at --max-share 50:
            one posting list of --meme-works works
  refused   the same with --refused-works works: more contributions than a call takes; the
            time of the refusal
  misquotes_ms   fs_misquotes over the host columns (median of --reps calls after a warm-up,
                 host clock around the synchronous call, the uploads and the copies out in it)
  passages_ms .. detail_ms
                 HIP-event times of its passes (fs_misquotes_times), medians over the same calls
  contributions, contributions_per_s
                 P, and P over the expand pass
  variants_ms, readings_ms
                 the yardsticks: fs_variants and fs_readings over the same columns in the same
                 process, the same way
  source         the hash of the library's sources the line was measured on (_lib.source_hash)
One line per row also goes to --out (default profiles/misquotes_bench.jsonl).

usage: python tools/misquotes_bench.py [--records N] [--reps R] [--mixes copied,meme,refused]
           [--meme-works W] [--refused-works W] [--oracle-max A]
           [--out profiles/misquotes_bench.jsonl] [--device D]
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

PASSES = ("passages_ms", "cells_ms", "number_ms", "postings_ms", "expand_ms", "place_ms",
          "detail_ms")
WRONG = N_SCRIPT            # spellings from here on are nobody's script word


def copied_records(n_works=4000, seed=1):
    """(work, fan_ix, orig_ix, spell): script word o is spelt o."""
    work, fan, orig = shared_records(n_works, seed)
    rng = np.random.default_rng(seed + 1)
    spell = orig.copy()
    wrong = WRONG
    first = np.searchsorted(work, np.arange(n_works + 1))
    w = 0
    while w < n_works:
        size = min(int(rng.integers(2, 51)), n_works - w)
        members = slice(first[w], first[w + size])
        for _ in range(int(rng.integers(1, 6))):
            o = orig[int(rng.integers(first[w], first[w + 1]))]
            hit = np.flatnonzero(orig[members] == o) + first[w]
            spell[hit] = wrong
            wrong += 1
        w += size
    typo = np.flatnonzero(rng.random(len(work)) < 0.02)
    spell[typo] = wrong + np.arange(len(typo))
    return (work, fan, orig, spell.astype(np.uint32)), wrong + len(typo)


def meme_records(n, sharing, find, seed=1):
    """The small mix, every record verbatim, and a passage of six words at the end of 2 *
    `sharing` active works: the first `sharing` with a wrong third word."""
    work, fan, orig = records(n, "small", seed)[:3]
    n_works = int(work[-1]) + 1
    same = np.arange(N_SCRIPT, dtype=np.uint32)
    base = find(work, fan, orig, orig, same, n_works, N_SCRIPT + 1)[0]
    active = np.flatnonzero(base["passage_records"])
    if len(active) < 2 * sharing:
        raise SystemExit("%d active works: fewer than %d" % (len(active), 2 * sharing))
    chosen = active[:2 * sharing]
    last = np.searchsorted(work, chosen, side="right") - 1
    add_work = np.repeat(chosen, 6)
    add_fan = np.repeat(fan[last].astype(np.int64) + 100, 6) + np.tile(np.arange(6), len(chosen))
    add_orig = np.tile(np.arange(7, 13), len(chosen))
    add_spell = add_orig.copy()
    add_spell[2:6 * sharing:6] = WRONG
    cols = [np.concatenate([a, b]).astype(np.int64) for a, b in
            ((work, add_work), (fan, add_fan), (orig, add_orig), (orig, add_spell))]
    order = np.lexsort((cols[1], cols[0]))
    return tuple(c[order].astype(np.uint32) for c in cols), len(active), n_works


def median(values):
    return round(float(np.median(values)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mixes", default="copied,meme,refused")
    ap.add_argument("--meme-works", type=int, default=5000)
    ap.add_argument("--refused-works", type=int, default=6000)
    ap.add_argument("--oracle-max", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "misquotes_bench.jsonl"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()

    from fandom_search_amd import _lib, abi, misquotes, readings, variants
    L = _lib.load()

    def find(*a, **kw):
        return misquotes.find_misquotes(*a, device=args.device, **kw)
    lines = []
    for mix in args.mixes.split(","):
        if mix == "copied":
            cols, n_spell = copied_records()
            n_works = int(cols[0][-1]) + 1
            active = None
        else:
            sharing = args.meme_works if mix == "meme" else args.refused_works
            cols, active, n_works = meme_records(args.records, sharing, find)
            n_spell = WRONG + 1
        n = len(cols[0])
        same = np.arange(N_SCRIPT, dtype=np.uint32)
        res = {"source": _lib.source_hash(), "mix": mix, "records": n, "works": n_works,
               "reps": args.reps}
        works = np.zeros(n_works, dtype=abi.MISQUOTE_WORK_DTYPE)
        if mix == "refused":
            res["active"] = active
            res["contributions"] = sharing * (sharing - 1) // 2
            found = np.zeros(1, dtype=abi.MISQUOTE_DTYPE)
            pairs = np.zeros(1, dtype=abi.MISQUOTE_PAIR_DTYPE)
        else:
            host = find(*cols, same, n_works, n_spell)                    # sizes the buffers
            works, found, pairs = host
            k = found["works"][found["telling"] > 0].astype(np.int64)
            res.update(active=int((works["passage_records"] > 0).sum()), misquotes=len(found),
                       telling=len(k), longest_list=int(k.max()) if len(k) else 0,
                       contributions=int((k * (k - 1) // 2).sum()), pairs=len(pairs))
            found, pairs = np.zeros_like(found), np.zeros_like(pairs)
        got = [C.c_uint64(0), C.c_uint64(0)]

        def call():
            return L.fs_misquotes(
                args.device, *(abi.ptr(c, C.c_uint32) for c in cols), abi.ptr(same, C.c_uint32), n,
                n_works, N_SCRIPT, n_spell, 6, 0, 2, 50, abi.FS_MISQUOTES_RARITY, 1, 1,
                works.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p), len(found),
                C.byref(got[0]), pairs.ctypes.data_as(C.c_void_p), len(pairs), C.byref(got[1]))
        want = abi.FS_E_UNSUPPORTED if mix == "refused" else abi.FS_OK
        assert call() == want, L.fs_last_error()                          # the warm-up
        total, passes = [], []
        for _ in range(args.reps):
            ms = (C.c_double * 8)()
            t = time.perf_counter()
            rc = call()
            total.append((time.perf_counter() - t) * 1e3)
            assert rc == want
            L.fs_misquotes_times(ms)
            passes.append(list(ms))
        if mix == "refused":
            res["refusal_ms"] = median(total)
            res["error"] = L.fs_last_error().decode()
        else:
            res["misquotes_ms"] = median(total)
            for j, name in enumerate(PASSES):
                res[name] = median([p[j] for p in passes])
            res["contributions_per_s"] = float("%.4g" % (
                res["contributions"] / (res["expand_ms"] * 1e-3))) if res["expand_ms"] > 0 else None
            for a, b in zip((works, found, pairs), host):                 # the timed calls' output
                assert len(a) == len(b) and (a == b).all()
            # the yardsticks
            vt, rt = [], []
            for j in range(args.reps + 1):
                t = time.perf_counter()
                variants.find_variants(cols[0], cols[2], cols[3], n_works, N_SCRIPT, n_spell,
                                       args.device)
                vt.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                readings.find_readings(*cols, n_works, N_SCRIPT, n_spell, device=args.device)
                rt.append((time.perf_counter() - t) * 1e3)
            res["variants_ms"], res["readings_ms"] = median(vt[1:]), median(rt[1:])
            if res["active"] <= args.oracle_max:
                from tests import misquotes_restated as mr
                recs = list(zip(*(c.tolist() for c in cols)))
                t = time.perf_counter()
                oracle = mr.misquotes(recs, same.tolist(), n_works, n_spell)
                res["oracle_s"] = round(time.perf_counter() - t, 3)
                for a, b, keys in zip(host, oracle,
                                      (mr.WORK_KEYS, mr.MISQUOTE_KEYS, mr.PAIR_KEYS)):
                    assert len(a) == len(b)
                    for name in keys:
                        assert a[name].tolist() == [d[name] for d in b], name
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
