"""`fanon` without a GPU: the restatement (tests/fanon_restated.py) against a brute force over
all substrings on tiny inputs, the command line's refusals, the host's ordering, --top and
decoding with the restatement standing in for the library, the token indices against
read_work_tokens, the pool against the plain loop, and the committed golden files."""

import os
import random

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, fanon, search
from tests import fanon_restated as fr
from tests.golden import make_fanon_golden as mfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- the restatement against a brute force ----------------------------------------------------

def brute(works, k, min_works):
    """Passages as (work, start, n_tokens, least, most), phrase sizes, and per work (shared
    positions, shared tokens), by looking at every substring and scanning every work for it."""
    def holders(seq):
        return [w for w, ids in enumerate(works)
                if any(ids[p:p + len(seq)] == seq for p in range(len(ids) - len(seq) + 1))]

    def shared(w, p):
        ids = works[w]
        return 0 <= p and p + k <= len(ids) and len(holders(ids[p:p + k])) >= min_works
    passages = []
    for w, ids in enumerate(works):
        for p in range(len(ids)):
            for n in range(k, len(ids) - p + 1):
                inside = all(shared(w, q) for q in range(p, p + n - k + 1))
                if inside and not shared(w, p - 1) and not shared(w, p + n - k + 1):
                    counts = [len(holders(ids[q:q + k])) for q in range(p, p + n - k + 1)]
                    passages.append((w, p, n, min(counts), max(counts)))
    groups = []
    for j, (w, p, n, _, _) in enumerate(passages):
        for g in groups:
            w0, p0, n0 = passages[g[0]][:3]
            if works[w0][p0:p0 + n0] == works[w][p:p + n]:
                g.append(j)
                break
        else:
            groups.append([j])
    per_work = []
    for w, ids in enumerate(works):
        positions = [p for p in range(len(ids)) if shared(w, p)]
        tokens = [t for t in range(len(ids)) if any(p <= t < p + k for p in positions)]
        per_work.append((len(positions), len(tokens)))
    return passages, groups, per_work


@pytest.mark.parametrize("k", [2, 3])
def test_restatement_against_brute_force(k):
    rng = random.Random(5 + k)
    for _ in range(12):
        works = [[rng.randrange(3) for _ in range(rng.randint(0, 12))] for _ in range(4)]
        for min_works in range(1, 6):
            records, grams, passages, phrases, totals = fr.fanon(works, [], k, min_works, 100)
            b_passages, b_groups, b_work = brute(works, k, min_works)
            assert [(p['work'], p['start'], p['n_tokens'], p['least'], p['most'])
                    for p in passages] == b_passages
            assert [[j for j, p in enumerate(passages) if p['phrase'] == r]
                    for r in range(len(phrases))] == b_groups
            for f, g in zip(phrases, b_groups):
                first = passages[g[0]]
                assert (f['work'], f['start'], f['n_tokens']) == \
                    (first['work'], first['start'], first['n_tokens'])
                assert f['n_passages'] == len(g)
                assert f['n_works'] == len({passages[j]['work'] for j in g})
            assert [(r['shared_positions'], r['shared_tokens']) for r in records] == b_work
            assert [r['n_passages'] for r in records] == \
                [sum(1 for p in b_passages if p[0] == w) for w in range(4)]
            assert totals['positions'] == sum(max(0, len(w) - k + 1) for w in works)
            for g in grams:
                seq = works[g['work']][g['start']:g['start'] + k]
                assert g['occurrences'] == sum(
                    1 for ids in works for p in range(len(ids) - k + 1) if ids[p:p + k] == seq)


def test_restatement_canon_and_common_by_hand():
    a, b = [1, 2, 3], [4, 5, 6]
    works = [a + [9] + b, a + [8] + b, b + [7], [0]]
    records, grams, passages, phrases, _ = fr.fanon(works, [[2, 3, 1, 2, 3], [1, 2]], 3, 2, 100)
    assert [(g['work'], g['start'], g['works']) for g in grams] == [(0, 4, 3)]
    assert [r['canon_positions'] for r in records] == [1, 1, 0, 0]
    assert [r['canon_tokens'] for r in records] == [3, 3, 0, 0]
    # b stands in 3 of 4 works: common at 74, not at 75
    assert [g['works'] for g in fr.fanon(works, [], 3, 2, 75)[1]] == [2, 3]
    assert [g['works'] for g in fr.fanon(works, [], 3, 2, 74)[1]] == [2]
    assert [r['common_positions'] for r in fr.fanon(works, [], 3, 2, 74)[0]] == [1, 1, 1, 0]
    with pytest.raises(ValueError):
        fr.fanon(works, [], 1)
    with pytest.raises(ValueError):
        fr.fanon(works, [], 33)


# ---- the command line -------------------------------------------------------------------------

@pytest.mark.parametrize("options, message", [
    (["--length", "1"], "--length must be from 2 to 32"),
    (["--length", "33"], "--length must be from 2 to 32"),
    (["--min-works", "0"], "--min-works must be at least 1"),
    (["--max-share", "0"], "--max-share must be from 1 to 100"),
    (["--max-share", "101"], "--max-share must be from 1 to 100"),
    (["--top", "-1"], "--top must be at least 0")])
def test_cli_refuses_before_any_file_is_read(options, message):
    with pytest.raises(SystemExit) as e:
        cli.main(["fanon", "no/such/directory"] + options)
    assert str(e.value) == "ao3.py fanon: error: " + message


def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["fanon", "runs/works/"])
    assert (args.length, args.min_works, args.max_share, args.keep_case, args.top) == \
        (8, 2, 100, False, 1000)
    assert (args.num_works, args.skip_works, args.listing, args.device, args.scripts) == \
        (-1, 0, None, 0, [])
    assert fanon.output_names(args.fan_works, args.output) == (
        "works-fanon.csv", "works-fanon-passages.csv", "works-fanon-grams.csv",
        "works-fanon-works.csv")
    args = cli.ao3_parser().parse_args(["fanon", "w", "a.txt", "b.txt", "-o", "out/x", "-n", "5",
                                        "-s", "2", "--listing", "os", "--keep-case"])
    assert args.scripts == ["a.txt", "b.txt"] and (args.num_works, args.skip_works) == (5, 2)
    assert fanon.output_names("w", "out/x")[0] == "out/x-fanon.csv"
    assert "fanon" in cli.ao3_parser().format_help()
    assert "fanon" not in [a for a in cli.full_parser()._subparsers._group_actions[0].choices]


def test_abi_names_the_unit():
    assert "fanon" in _lib.TIMED
    assert {"fs_fanon", "fs_fanon_dev", "fs_fanon_times"} <= set(_lib.SYMBOLS)
    assert len(abi.FANON_MS_NAMES) == 7
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    for name, size in (("work", 40), ("gram", 16), ("passage", 24), ("phrase", 32)):
        assert getattr(abi, "FANON_%s_DTYPE" % name.upper()).itemsize == size
        assert "} fs_fanon_%s;" % name in text
    assert "#define FS_FANON_TILE %uu" % abi.FS_FANON_TILE in text
    assert "#define FS_FANON_MAX_BYTES (8ull << 30)" in text and abi.FS_FANON_MAX_BYTES == 8 << 30


# ---- the host around the library, the restatement standing in for it ---------------------------

def restated_engine(tok, work_off, n_ids, canon, canon_off, length, min_works, max_share,
                    device=0):
    off = [int(o) for o in work_off]
    works = [[int(t) for t in tok[off[w]:off[w + 1]]] for w in range(len(off) - 1)]
    coff = [int(o) for o in canon_off]
    scripts = [[int(t) for t in canon[coff[s]:coff[s + 1]]] for s in range(len(coff) - 1)]
    assert all(t < n_ids for w in works for t in w)
    parts = fr.fanon(works, scripts, length, min_works, max_share)
    out = []
    for part, keys, dt in zip(parts[:4], (fr.WORK_KEYS, fr.GRAM_KEYS, fr.PASSAGE_KEYS,
                                          fr.PHRASE_KEYS),
                              (abi.FANON_WORK_DTYPE, abi.FANON_GRAM_DTYPE,
                               abi.FANON_PASSAGE_DTYPE, abi.FANON_PHRASE_DTYPE)):
        a = np.zeros(len(part), dtype=dt)
        for name in keys:
            a[name] = [d[name] for d in part]
        out.append(a)
    return tuple(out) + (parts[4],)


@pytest.mark.parametrize("options", [[], ["--top", "2"], ["--top", "0", "--length", "3"],
                                     ["--length", "4", "--min-works", "3", "--keep-case"],
                                     ["--max-share", "50", "--top", "1"]])
def test_host_ordering_top_and_text(monkeypatch, tmp_path, options):
    from fandom_search_amd import engine
    monkeypatch.setattr(engine, "fanon", restated_engine)
    monkeypatch.setenv("FANDOM_SEARCH_WORKERS", "0")
    monkeypatch.chdir(ROOT)
    prefix = str(tmp_path / "x")
    cli.main(["fanon", mfg.WORKS, mfg.SCRIPT, "-o", prefix] + options)
    want = fr.tables(mfg.WORKS, [mfg.SCRIPT], **mfg.restated_options(options))
    for suffix, head, rows in zip(fr.SUFFIXES, fr.HEADS, want):
        assert fr.read_csv(prefix + suffix) == fr.csv_text(head, rows), suffix
    phrases, passages = want[0], want[1]
    assert [r[0] for r in phrases] == list(range(1, len(phrases) + 1))
    keys = [(-r[2], -r[5], -r[1]) for r in phrases]
    assert keys == sorted(keys)
    if options[:2] == ["--top", "2"]:
        assert len(phrases) == 2 and any(r[4] == '' for r in passages)
        assert len(want[3]) == 9                       # every work, whatever --top says


def test_rank_is_a_stable_sort():
    f = np.zeros(5, dtype=abi.FANON_PHRASE_DTYPE)
    f['n_works'] = [2, 3, 2, 2, 3]
    f['most'] = [5, 1, 5, 6, 1]
    f['n_tokens'] = [9, 4, 9, 2, 8]
    assert fanon.rank_phrases(f).tolist() == [4, 1, 3, 0, 2]
    g = np.zeros(4, dtype=abi.FANON_GRAM_DTYPE)
    g['works'] = [2, 2, 3, 2]
    g['occurrences'] = [4, 7, 3, 4]
    assert fanon.rank_grams(g).tolist() == [2, 1, 0, 3]


def test_token_indices_are_those_of_read_work_tokens(tmp_path):
    text = "\n\n  Hello --  there, \"General\" Kenobi!\n\n\nYou are a bold one...\n\n"
    other = "HELLO there.\n"
    for name, t in (("a.txt", text), ("b.txt", other)):
        (tmp_path / name).write_text(t, encoding="utf-8")
    names = [str(tmp_path / "a.txt"), str(tmp_path / "b.txt")]
    c = fanon.Corpus(names, workers=0)
    toks = [search.read_work_tokens(n) for n in names]
    assert c.work_off.tolist() == [0, len(toks[0]), len(toks[0]) + len(toks[1])]
    for w, t in enumerate(toks):
        assert [c.text(w, i, 1) for i in range(len(t))] == t
        assert c.text(w, 2, 3) == ' '.join(t[2:5])
    ids = c.tok()
    assert ids[0] == ids[len(toks[0])]                         # Hello and HELLO fold together
    assert fanon.Corpus(names, keep_case=True, workers=0).tok()[0] != \
        fanon.Corpus(names, keep_case=True, workers=0).tok()[len(toks[0])]
    assert c.n_ids == len({t.lower() for ts in toks for t in ts})
    assert c.script_ids(["hello", "Kenobi", "nowhere"]).tolist()[2] == abi.FS_FANON_NO_ID
    assert c.script_ids(["hello"])[0] == ids[0]
    assert len(c.texts) == len(set(c.texts))                   # every text held once


def test_pool_and_plain_loop_read_the_same(tmp_path):
    rng = random.Random(3)
    words = "the force is strong with this one , always . Hope".split()
    for i in range(70):
        (tmp_path / ("w%02d.txt" % i)).write_text(
            ' '.join(rng.choice(words) for _ in range(rng.randint(0, 30))), encoding="utf-8")
    names = search.list_fan_works(str(tmp_path))
    plain, pooled = fanon.Corpus(names, workers=0), fanon.Corpus(names, workers=2)
    assert plain.texts == pooled.texts and plain.n_ids == pooled.n_ids
    assert plain.raw.tobytes() == pooled.raw.tobytes()
    assert plain.work_off.tobytes() == pooled.work_off.tobytes()
    assert plain.tok().tobytes() == pooled.tok().tobytes()


# ---- the golden files --------------------------------------------------------------------------

def test_golden_files_are_what_the_restatement_gives(monkeypatch):
    monkeypatch.chdir(ROOT)
    built = mfg.build()
    assert len(built) == 12
    for name, text in built.items():
        assert fr.read_csv(os.path.join(GOLDEN, name)) == text, name
    # the three option sets differ where they should
    works = {case: built[mfg.golden_names(case)[3]] for case, _, _ in mfg.CASES}
    assert works["default"] != works["share50_script"] != works["k4_w3_case"]
    for name in os.listdir(os.path.join(GOLDEN, "fanon_works")):
        assert os.path.getsize(os.path.join(GOLDEN, "fanon_works", name)) < 4096
