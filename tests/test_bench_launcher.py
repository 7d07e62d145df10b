"""bench.py --gpus N typed without a launcher starts its own ranks: the
decision is a pure function (tested here without a GPU); with a GPU the command itself
runs two ranks over gloo on the one card and must print one JSON line."""

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_launcher_decision():
    b = _bench()
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    cmd = b.launcher_command(b.parse(argv), argv, {}, port=29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29555"
    assert cmd[-7] == os.path.join(ROOT, "bench.py") and cmd[-6:] == argv
    # a rank under a launcher, and N = 1, run in this process
    assert b.launcher_command(b.parse(argv), argv, {"WORLD_SIZE": "8"}) is None
    assert b.launcher_command(b.parse(["--gpus", "1"]), ["--gpus", "1"], {}) is None
    assert b.launcher_command(b.parse([]), [], {}) is None
    # an image that merely exports WORLD_SIZE=1 has not launched anything
    assert b.launcher_command(b.parse(argv), argv, {"WORLD_SIZE": "1"}) is not None
    assert b.launcher_command(b.parse(argv), argv, {"WORLD_SIZE": "1", "RANK": "0"}) is None
    # no port given: the launcher's own rendezvous finds a free one
    cmd = b.launcher_command(b.parse(argv), argv, {})
    assert "--standalone" in cmd and cmd[cmd.index("--local-addr") + 1] == "127.0.0.1"
    assert "--master-port" not in cmd


def test_defaults_follow_the_contract():
    b = _bench()
    a = b.parse([])
    assert a.gpus == 1 and a.scaling == ""      # N = 1: c2; N > 1: configs[2] split N ways (strong)
    # a plain run times exactly --steps steps, once, and measures nothing beside the headline
    assert a.reps == 1 and not a.full and a.dump_outputs == ""
    assert b.parse(["--full", "--dump-outputs", "d"]).full


def _rows(n, seed):
    from fandom_search_amd import abi
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=abi.ROW_DTYPE)
    for name in ("work", "fan_ix", "orig_ix", "lev"):
        rows[name] = rng.integers(0, 40, n)
    rows["dist"] = rng.random(n)
    rows["comb"] = rng.random(n) - 0.5
    return rows


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_is_canonical_float64(tmp_path):
    """The records land in a device buffer in an order that depends on scheduling: the dump
    is the same for any order, float64, sorted, and holds every record exactly."""
    b = _bench()
    rows = _rows(3000, 1)
    b.dump_outputs(str(tmp_path / "a"), [rows])
    b.dump_outputs(str(tmp_path / "b"), [rows[np.random.default_rng(2).permutation(len(rows))]])
    a, c = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(rows.dtype.names + ("n_rows",))
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], c[k]), k
    assert a["n_rows"].tolist() == [len(rows)]
    back = np.zeros(len(rows), dtype=rows.dtype)
    for k in rows.dtype.names:
        back[k] = a[k]
    assert np.array_equal(np.sort(back), np.sort(rows))
    keys = list(zip(*(a[k] for k in rows.dtype.names)))
    assert keys == sorted(keys)


def test_dump_outputs_ranks_and_size_cap(tmp_path, monkeypatch):
    """Several ranks' records carry `rank`; beyond the byte budget a fixed seeded sample of the
    sorted records is written, the full count beside it."""
    b = _bench()
    parts = [_rows(500, 3), _rows(700, 4)]
    b.dump_outputs(str(tmp_path / "r"), parts)
    r = _load(tmp_path / "r")
    assert r["n_rows"].tolist() == [1200] and len(r["rank"]) == 1200
    assert (r["rank"] == 0).sum() == 500 and (r["rank"] == 1).sum() == 700
    monkeypatch.setattr(b, "DUMP_BYTES", 7 * 8 * 100)
    b.dump_outputs(str(tmp_path / "s1"), parts)
    b.dump_outputs(str(tmp_path / "s2"), parts[::-1])
    s1, s2 = _load(tmp_path / "s1"), _load(tmp_path / "s2")
    assert s1["n_rows"].tolist() == [1200] and len(s1["work"]) == 100
    assert np.array_equal(s1["work"], s2["work"]) and np.array_equal(s1["comb"], s2["comb"])
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) < 64 << 20


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("gather_root,scaling", [("rotate", ""), ("step", ""), ("0", ""), ("rotate", "weak")])
def test_bench_starts_its_own_ranks(tmp_path, gather_root, scaling):
    """`python bench.py --gpus 2 ...` exactly as the driver types it (no launcher): two ranks
    (gloo between them, both on this one GPU), one JSON line from rank 0, the records every
    rank sent checked on the rank that received the last step -- for the all_to_all per N
    steps (default), a gather per step with the root going round, and a gather to rank 0.
    That check is one of --full's; the last step's records are dumped by the rank that holds them."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--works", "200", "--steps", "3", "--warmup", "1", "--reps", "2", "--full",
                        "--dump-outputs", str(tmp_path / "out"),
                        "--gather-root", gather_root] + (["--scaling", scaling] if scaling else []),
                       env=env, cwd=str(tmp_path), timeout=800, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    # typed as is, N > 1 measures configs[2] (100k works x 5k tokens) split over the ranks
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == (scaling or "strong")
    assert d["config"]["tokens_per_work"] == (2000 if scaling == "weak" else 5000)
    assert d["config"]["gather_verified"] is True
    assert d["value"] > 0 and len(d["samples_ms"]) == 2
    out = _load(tmp_path / "out")
    n = int(out["n_rows"][0])
    assert n > 0 and len(out["rank"]) == len(out["work"]) == n
    assert set(np.unique(out["rank"]).tolist()) <= {0.0, 1.0}


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dump_outputs_are_the_last_steps_records(tmp_path):
    """A plain N = 1 run with --dump-outputs: the records of its last timed step are those a
    search of that step's batch returns (the steps rotate over the distinct batches), and a
    second run with the same arguments writes the same files."""
    from fandom_search_amd import abi, synth, vocab
    from fandom_search_amd.engine import ScriptIndex
    works, steps, warmup = 200, 4, 2          # (the last step searches batch 1 of 4)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--works", str(works),
                            "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / tag)],
                           env=env, cwd=str(tmp_path), timeout=500, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["ms_per_step"] > 0 and len(d["samples_ms"]) == 1
        assert "roofline" not in d and "companions" not in d and "cpu_baseline" not in d
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # the batch of the last step: batches rotate, batch r holds works [r * works, (r + 1) * works)
    conf = synth.CONFIGS["c2"]
    rotate = d["config"]["distinct_batches"]
    last = (warmup + steps - 1) % rotate
    words, emb = synth.vocab_words(), synth.embedding()
    script = synth.script_tokens(conf["script_tokens"])
    tok, off = synth.corpus_tokens(works, conf["tokens_per_work"], script, first_work=last * works)
    chars, coff = vocab.pack_strings(words)
    ix = ScriptIndex(script, [words[int(t)] for t in script], emb, synth.lsh_normals(6),
                     cfg=abi.make_config(window_size=6, device=0))
    c = ix.corpus(tok, off, chars, coff)
    rows, _ = ix.search(c)
    c.close()
    ix.close()
    _bench().dump_outputs(str(tmp_path / "want"), [rows])
    want = _load(tmp_path / "want")
    assert len(rows) > 0 and sorted(want) == sorted(a)
    for k in want:
        assert np.array_equal(a[k], want[k]), k
