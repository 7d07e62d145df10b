"""Match-record layouts for the matrix tests: (work name, fan_ix, orig_ix) lists, hand-made for
the shapes the span rule turns on and seeded random ones.  Shared by the host and the GPU test."""

import random


def span(work, f0, o0, length):
    return [(work, f0 + k, o0 + k) for k in range(length)]


def fan_run(work, f0, origs):
    """One fan run (consecutive fan indices) naming the script words `origs` in that order."""
    return [(work, f0 + k, o) for k, o in enumerate(origs)]


def shaped():
    """{name: records}: repeated script words with c = 2, 3, 4 at the start, in the middle and
    at the end of a span, script order scrambled inside a fan run, repeated fan indices, ties."""
    out = {}
    for c in (2, 3, 4):
        out["dup%d_start" % c] = fan_run("a", 0, [10] * c + [11, 12, 13, 14]) + span("b", 0, 9, 6)
        out["dup%d_middle" % c] = fan_run("a", 0, [10, 11] + [12] * c + [13, 14, 15]) + \
            span("b", 3, 11, 4)
        out["dup%d_end" % c] = fan_run("a", 0, [10, 11, 12, 13] + [14] * c) + span("b", 0, 12, 5)
        out["dup%d_alone" % c] = fan_run("a", 0, [20] * c)
    out["scrambled"] = fan_run("a", 0, [10, 12, 11]) + fan_run("b", 5, [7, 6, 5, 9, 8, 6]) + \
        fan_run("c", 0, [12, 11, 10, 13])
    # a repeated fan index splits a run; so does a gap
    out["fan_repeat"] = [("a", 0, 10), ("a", 1, 11), ("a", 1, 12), ("a", 2, 13), ("a", 3, 14),
                         ("a", 5, 15), ("a", 6, 16), ("a", 7, 17)]
    # equal counts inside a span: the first wins
    out["tie_inside"] = span("a", 0, 10, 6) + span("b", 0, 10, 6)
    # an equal count in front of the start: dropped; behind it: kept
    out["tie_before"] = span("a", 0, 10, 4) + span("b", 0, 12, 4) + span("c", 0, 14, 4)
    out["tie_after"] = span("a", 0, 10, 3) + span("b", 0, 11, 3) + span("b", 9, 11, 3) + \
        span("c", 0, 13, 3)
    # starts below n - 1 and within n of the script's end
    out["edges"] = span("a", 0, 0, 5) + span("b", 0, 1, 4) + span("c", 7, 0, 3)
    # file order shuffled: works interleaved, fan order reversed
    rows = span("a", 0, 3, 5) + span("b", 2, 4, 4) + fan_run("a", 9, [8, 8, 9, 7])
    out["shuffled"] = rows[::-1]
    return out


def random_records(seed, n_works=6, n_script=40):
    """Seeded random records in shuffled file order: fan runs whose script words step by 0, 1 or
    2, some scrambled, some with a repeated fan index."""
    rnd = random.Random(seed)
    rows = []
    for w in range(rnd.randint(1, n_works)):
        f = rnd.randint(0, 5)
        for _ in range(rnd.randint(1, 4)):
            o = rnd.randint(0, n_script - 12)
            origs = []
            for _ in range(rnd.randint(1, 10)):
                origs.append(o)
                o = min(n_script - 1, o + rnd.choice((0, 0, 1, 1, 1, 1, 2)))
            if rnd.random() < 0.4:
                rnd.shuffle(origs)
            for o in origs:
                rows.append(("w%d" % w, f, o))
                f += rnd.choice((0, 1, 1, 1, 1, 1, 1, 2))
            f += rnd.randint(0, 3)
    if rnd.random() < 0.7:
        rnd.shuffle(rows)
    return rows
