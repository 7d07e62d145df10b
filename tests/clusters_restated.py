"""The `clusters` contract restated in plain Python, a set of script words per work: the oracle
of the tests (tests/test_clusters_host.py, tests/test_gpu_clusters.py) and of the committed
tests/golden/clusters_*.csv.  The product never imports it."""

import csv
import io

from tests import pairs_restated as pp
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
CLUSTER_FIELDS = ['CLUSTER', 'WORKS', 'LINKS', 'HUB_FAN_WORK_FILENAME', 'HUB_LINKS',
                  'COVERED_WORDS', 'COMMON_WORDS', 'PEAK_WORKS', 'PEAK_WORD_INDEX',
                  'COMMON_RUN_START', 'COMMON_RUN_WORDS', 'COMMON_RUN_CHARACTER',
                  'COMMON_RUN_SCENE', 'COMMON_RUN_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'CLUSTER', 'CLUSTER_WORKS', 'COVERED_WORDS', 'LINKS',
               'BEST_PARTNER', 'BEST_SHARED_WORDS']
WORK_KEYS = ['covered', 'root', 'size', 'cluster', 'links', 'best', 'best_shared']
CLUSTER_KEYS = ['root', 'n_works', 'n_links', 'hub', 'hub_links', 'covered', 'common', 'peak',
                'peak_first', 'run_first', 'run_words']
UNKNOWN_WORD = pp.UNKNOWN_WORD


def linked(ca, cb, min_shared, min_jaccard):
    """Whether the coverages ca and cb (sets) are linked, and their shared words."""
    shared = len(ca & cb)
    return (shared >= min_shared and
            100 * shared >= min_jaccard * (len(ca) + len(cb) - shared)), shared


def clusters(records, n_works, n_script, min_words=6, max_gap=0, min_shared=6, min_jaccard=50,
             min_size=2, common_pct=50):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).
    Returns (one dict of WORK_KEYS per work, one dict of CLUSTER_KEYS per listed family in
    ascending order of root)."""
    if min_words < 1 or min_shared < 1 or min_size < 1 or not 1 <= common_pct <= 100:
        raise ValueError("min_words, min_shared, min_size and common_pct must be at least 1")
    if not 0 <= min_jaccard <= 100:
        raise ValueError("min_jaccard is a percentage")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = pp.coverage(records, n_works, min_words, max_gap)
    works = [dict(covered=len(c), root=NONE, size=0, cluster=NONE, links=0, best=NONE,
                  best_shared=0) for c in cov]
    active = [w for w in range(n_works) if cov[w]]
    family = {w: {w} for w in active}                    # work -> the set it is in (shared)
    for i, a in enumerate(active):
        for b in active[i + 1:]:
            link, shared = linked(cov[a], cov[b], min_shared, min_jaccard)
            if not link:
                continue
            for w, other in ((a, b), (b, a)):
                works[w]['links'] += 1
                if (shared, -other) > (works[w]['best_shared'], -works[w]['best']):
                    works[w]['best'], works[w]['best_shared'] = other, shared
            if family[a] is not family[b]:
                merged = family[a] | family[b]
                for w in merged:
                    family[w] = merged
    out = []
    for root in active:
        members = sorted(family[root])
        if members[0] != root:
            continue
        listed = len(members) >= min_size
        for w in members:
            works[w]['root'], works[w]['size'] = root, len(members)
            if listed:
                works[w]['cluster'] = len(out)
        if not listed:
            continue
        depth = {}
        for w in members:
            for o in cov[w]:
                depth[o] = depth.get(o, 0) + 1
        t = (common_pct * len(members) + 99) // 100
        common = {o for o, d in depth.items() if d >= t}
        peak = max(depth.values())
        run = pp.longest_run(common) if common else (NONE, 0)
        hub = min(members, key=lambda w: (-works[w]['links'], w))
        out.append(dict(root=root, n_works=len(members),
                        n_links=sum(works[w]['links'] for w in members) // 2, hub=hub,
                        hub_links=works[hub]['links'], covered=len(depth), common=len(common),
                        peak=peak, peak_first=min(o for o, d in depth.items() if d == peak),
                        run_first=run[0], run_words=run[1]))
    return works, out


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def clusters_csv(text, min_words=6, max_gap=0, min_shared=6, min_jaccard=50, min_size=2,
                 common_pct=50):
    """The bytes `ao3.py clusters` writes for a match CSV's text: (clusters, clusters-works)."""
    rows = pr.read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4])) for w, f, k in keyed]
    names = list(work_of)
    label = {}
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        if label.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
    n_script = max(label) + 1 if label else 0
    works, found = clusters(recs, len(names), n_script, min_words, max_gap, min_shared,
                            min_jaccard, min_size, common_pct)
    unknown = (UNKNOWN_WORD, '', '')
    # the largest family first, then the smaller root
    ranked = sorted(range(len(found)), key=lambda k: (-found[k]['n_works'], found[k]['root']))
    rank = {k: i + 1 for i, k in enumerate(ranked)}
    ctab = [CLUSTER_FIELDS]
    for k in ranked:
        c = found[k]
        s, n = c['run_first'], c['run_words']
        # without a common word: no start, character, scene or text, and a run of 0 words
        run = ['', 0, '', '', ''] if not c['common'] else [
            s, n, label.get(s, unknown)[1], label.get(s, unknown)[2],
            ' '.join(label.get(o, unknown)[0] for o in range(s, s + n))]
        ctab.append([rank[k], c['n_works'], c['n_links'], names[c['hub']], c['hub_links'],
                     c['covered'], c['common'], c['peak'], c['peak_first']] + run)
    wtab = [WORK_FIELDS]
    for w, v in enumerate(works):
        if v['covered']:
            wtab.append([names[w], '' if v['cluster'] == NONE else rank[v['cluster']], v['size'],
                         v['covered'], v['links'],
                         '' if v['best'] == NONE else names[v['best']], v['best_shared']])
    return _csv(ctab), _csv(wtab)
