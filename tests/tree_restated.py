"""The `tree` contract restated in plain Python, a set of script words per work: the oracle of
the tests (tests/test_tree_host.py, tests/test_gpu_tree.py) and of the committed
tests/golden/tree_*.csv.  Coverages as Python sets, every pair of works, the whole edge list
sorted by the order, Kruskal.  The product never imports it."""

import csv
import io

from tests import pairs_restated as pp
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
MERGE_FIELDS = ['MERGE', 'LEVEL', 'A_FAN_WORK_FILENAME', 'B_FAN_WORK_FILENAME', 'SHARED_WORDS',
                'A_COVERED_WORDS', 'B_COVERED_WORDS', 'LEFT', 'RIGHT', 'LEFT_WORKS',
                'RIGHT_WORKS', 'WORKS', 'FIRST_FAN_WORK_FILENAME', 'TREE', 'SHARED_RUN_START',
                'SHARED_RUN_WORDS', 'SHARED_RUN_CHARACTER', 'SHARED_RUN_SCENE',
                'SHARED_RUN_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'TREE', 'TREE_WORKS', 'EDGES',
               'JOINED_AT_MERGE', 'JOINED_AT_LEVEL', 'BEST_PARTNER', 'LEAF_ORDER']
LEVEL_FIELDS = ['LEVEL', 'MERGES', 'FAMILIES', 'LARGEST_WORKS', 'SINGLE_WORKS']
MERGE_KEYS = ['a', 'b', 'level', 'shared', 'a_covered', 'b_covered', 'left', 'right',
              'left_works', 'right_works', 'works', 'first_work', 'tree', 'run_first',
              'run_words']
WORK_KEYS = ['covered', 'tree', 'tree_works', 'edges', 'joined_merge', 'joined_level', 'best',
             'leaf']
LEVEL_KEYS = ['level', 'merges', 'merges_above', 'families', 'largest', 'joined', 'singles']
MEASURES = ('jaccard', 'shared')
UNKNOWN_WORD = pp.UNKNOWN_WORD


def level_of(measure, shared, ca, cb):
    """The level of an edge between works covering ca and cb words that share `shared`."""
    if measure == 'jaccard':
        return shared * 1000000 // (ca + cb - shared)
    if measure == 'shared':
        return shared
    raise ValueError("measure must be jaccard or shared")


def edges_of(cov, measure, min_shared, min_level):
    """Every edge (level, a, b, the shared words) in the order: the higher level first, then
    the smaller a, then the smaller b."""
    active = [w for w in range(len(cov)) if cov[w]]
    out = []
    for i, a in enumerate(active):
        for b in active[i + 1:]:
            both = cov[a] & cov[b]
            if len(both) < min_shared:
                continue
            level = level_of(measure, len(both), len(cov[a]), len(cov[b]))
            if level >= min_level:
                out.append((level, a, b, both))
    out.sort(key=lambda e: (-e[0], e[1], e[2]))
    return out


def tree(records, n_works, n_script, min_words=6, max_gap=0, measure='jaccard', min_shared=6,
         min_level=0):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).
    Returns (one dict of WORK_KEYS per work, one dict of MERGE_KEYS per merge in merge order,
    one dict of LEVEL_KEYS per level, the highest first); merges, trees and leaves count from
    0."""
    if min_words < 1 or min_shared < 1 or max_gap < 0:
        raise ValueError("min_words and min_shared must be at least 1, max_gap at least 0")
    if measure not in MEASURES:
        raise ValueError("measure must be jaccard or shared")
    if min_level < 0 or (measure == 'jaccard' and min_level > 1000000):
        raise ValueError("min_level outside the levels")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = pp.coverage(records, n_works, min_words, max_gap)
    works = [dict(covered=len(c), tree=NONE, tree_works=0, edges=0, joined_merge=NONE,
                  joined_level=0, best=NONE, leaf=NONE) for c in cov]
    active = [w for w in range(n_works) if cov[w]]
    # a family: its leaves in order and the merge that made it; shared by its works
    family = {w: dict(leaves=[w], made=NONE) for w in active}
    merges, levels = [], []
    for level, a, b, both in edges_of(cov, measure, min_shared, min_level):
        left, right = family[a], family[b]
        if left is right:
            continue
        k = len(merges)
        run = pp.longest_run(both)
        joined = dict(leaves=left['leaves'] + right['leaves'], made=k)
        merges.append(dict(a=a, b=b, level=level, shared=len(both), a_covered=len(cov[a]),
                           b_covered=len(cov[b]), left=left['made'], right=right['made'],
                           left_works=len(left['leaves']), right_works=len(right['leaves']),
                           works=len(joined['leaves']), first_work=min(joined['leaves']),
                           tree=NONE, run_first=run[0], run_words=run[1]))
        for w in joined['leaves']:
            family[w] = joined
        for w, other in ((a, b), (b, a)):
            works[w]['edges'] += 1
            if works[w]['joined_merge'] == NONE:
                works[w].update(joined_merge=k, joined_level=level, best=other)
        if not levels or levels[-1]['level'] != level:
            levels.append(dict(level=level, merges=0, merges_above=k))
        sizes = [len(f['leaves']) for f in {id(f): f for f in family.values()}.values()]
        big = [s for s in sizes if s >= 2]
        levels[-1].update(merges=levels[-1]['merges'] + 1, families=len(big), largest=max(big),
                          joined=sum(big), singles=len(sizes) - len(big))
    # the trees: most works first, then first appearance; the leaves tree by tree
    trees = sorted({id(f): f for f in family.values()}.values(),
                   key=lambda f: (-len(f['leaves']), min(f['leaves'])))
    leaf = 0
    for rank, f in enumerate(trees):
        for w in f['leaves']:
            works[w].update(tree=rank, tree_works=len(f['leaves']), leaf=leaf)
            leaf += 1
    for m in merges:
        m['tree'] = works[m['a']]['tree']
    return works, merges, levels


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def tree_csv(text, min_words=6, max_gap=0, measure='jaccard', min_shared=6, min_level=0):
    """The bytes `ao3.py tree` writes for a match CSV's text: (tree, tree-works,
    tree-levels)."""
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
    works, merges, levels = tree(recs, len(names), n_script, min_words, max_gap, measure,
                                 min_shared, min_level)
    unknown = (UNKNOWN_WORD, '', '')

    def side(k):
        return '' if k == NONE else k + 1

    mtab = [MERGE_FIELDS]
    for k, m in enumerate(merges):
        s, n = m['run_first'], m['run_words']
        mtab.append([k + 1, m['level'], names[m['a']], names[m['b']], m['shared'],
                     m['a_covered'], m['b_covered'], side(m['left']), side(m['right']),
                     m['left_works'], m['right_works'], m['works'], names[m['first_work']],
                     m['tree'] + 1, s, n, label.get(s, unknown)[1], label.get(s, unknown)[2],
                     ' '.join(label.get(o, unknown)[0] for o in range(s, s + n))])
    wtab = [WORK_FIELDS]
    for w, v in enumerate(works):
        if v['covered']:
            joined = ['', '', ''] if v['joined_merge'] == NONE else [
                v['joined_merge'] + 1, v['joined_level'], names[v['best']]]
            wtab.append([names[w], v['covered'], v['tree'] + 1, v['tree_works'], v['edges']]
                        + joined + [v['leaf']])
    ltab = [LEVEL_FIELDS] + [[v['level'], v['merges'], v['families'], v['largest'],
                              v['singles']] for v in levels]
    return _csv(mtab), _csv(wtab), _csv(ltab)
