"""Command line of the search path: the `search`, `format`, `matrix` and
`validate` sub-commands of the reference's ao3.py (/root/reference/ao3.py:509-526
and _deprecated.py:83-89), same positionals, flags and output files, and
`passages`, which joins a match CSV's per-word records into passages of reuse
(fandom_search_amd/passages.py), and `works`, which summarises them by fan work
(fandom_search_amd/works.py), and `quotes`, which ranks the stretches of the script by the works
that reuse them (fandom_search_amd/quotes.py), and `variants`, which ranks the fan spellings
under each script word (fandom_search_amd/variants.py), and `pairs`, which ranks the pairs of fan
works by the script words both quote (fandom_search_amd/pairs.py), and `groups`, which reduces
the reuse by year, author, language or tag of the works (fandom_search_amd/groups.py), and
`clusters`, which gathers the works quoting the same lines into families
(fandom_search_amd/clusters.py), and `readings`, which collates the wordings fans give each
quoted stretch (fandom_search_amd/readings.py), and `retellings`, which lists the works that
quote the script in the script's own order (fandom_search_amd/retellings.py), and `companions`,
which relates the quoted stretches of the script by the works quoting both
(fandom_search_amd/companions.py), and `transitions`, which counts which stretch the works
quote next after each stretch (fandom_search_amd/transitions.py), and `sources`, which joins
the match files of several scripts and says which script each fan passage quotes
(fandom_search_amd/sources.py), and `alignments`, which aligns every fan work against the script
with gaps, for quotes with inserted or dropped words (fandom_search_amd/alignments.py), and
`lines`, which ranks the lines of the script markup by the works quoting them and says how
completely each is quoted (fandom_search_amd/lines.py), and `fragments`, which lists the
phrases the works quote word for word, each with the works quoting it in full
(fandom_search_amd/fragments.py), and `fanon`, which reads the fan works themselves and lists
the phrases they share with each other and the script lacks (fandom_search_amd/fanon.py), and `digest`, which picks the fewest works that together show
everything the works quote (fandom_search_amd/digest.py), and `intervals`, which resamples the
works to say how sure the works-per-stretch counts are (fandom_search_amd/intervals.py), and
`contrast`, which says what one group of works quotes more than another and which of those
differences survive a look at every unit at once (fandom_search_amd/contrast.py), and
`saturation`, which says how much of what fans quote a sample of the works would have shown
(fandom_search_amd/saturation.py), and `trends`, which says which stretches the later works quote
more and which the earlier (fandom_search_amd/trends.py), and `neighbours`, which lists each
work's closest works by the rare lines both quote (fandom_search_amd/neighbours.py), and
`misquotes`, which lists the works that share departures from the script
(fandom_search_amd/misquotes.py), and `tree`, which shows how the families of works merge as
the bar drops (fandom_search_amd/tree.py), and `bundles`, which lists the sets of stretches
the same works quote (fandom_search_amd/bundles.py), and `routes`, which lists the sequences
of stretches the works quote in order (fandom_search_amd/routes.py).  The
reference's scrape / clean / getmeta / vis sub-commands are outside this package
(out of scope)."""

import argparse
import sys


class _Scripts(argparse.Action):
    """script [script ...]: args.scripts holds them all, args.script the first (what format,
    validate and a one-script search read)."""

    def __call__(self, parser, namespace, values, option_string=None):
        namespace.scripts = list(values)
        namespace.script = values[0]


_SPANS = (lambda a: a.min_words < 1 or a.max_gap < 0,
          '--min-words must be at least 1, --max-gap at least 0')
_SHARE = (lambda a: not 0 <= a.min_share <= 100, '--min-share must be from 0 to 100')


def _own(*flags, **kwargs):
    """An argument of one command, for _analysis to add at its place."""
    return flags, kwargs


def _analysis(subparsers, name, help, output_help, checks, first=(), middle=(), last=(),
              spans=True, several=False):
    """The sub-command `name` over a match csv (`several`: over two or more, with a required
    -o): the arguments every analysis command has -- matches, -o/--output, --min-words and
    --max-gap (`spans`), --device, --reader -- and the command's own (_own), those of `first`
    in front of -o, of `middle` behind it and of `last` behind --max-gap.  `checks` is what
    _command tests before it runs the command."""
    p = subparsers.add_parser(name, help=help)
    if several:
        p.add_argument('matches', action='store', nargs='+', metavar='matches',
                       help='filenames for search output (dated or batch files), one '
                            'per script, at least two')
    else:
        p.add_argument('matches', action='store',
                       help='filename for search output (dated or batch file)')
    for flags, kwargs in first:
        p.add_argument(*flags, **kwargs)
    p.add_argument('-o', '--output', action='store', default=None, required=several,
                   help=output_help)
    for flags, kwargs in middle:
        p.add_argument(*flags, **kwargs)
    if spans:
        p.add_argument('--min-words', default=6, type=int,
                       help='fewest matched words a passage has, default 6')
        p.add_argument('--max-gap', default=0, type=int,
                       help='words without a record a passage may step over on each '
                            'side at once, default 0')
    for flags, kwargs in last:
        p.add_argument(*flags, **kwargs)
    p.add_argument('--device', default=0, type=int, help='HIP device ordinal')
    p.add_argument('--reader', default=None, choices=('device', 'python'),
                   help='who reads the match %s: the GPU (default) or csv.reader; also '
                        'FANDOM_SEARCH_READER' % ('csvs' if several else 'csv'))

    def func(args):
        return _command(name, checks, args)
    func.__name__ = '_' + name          # (what the command's function was called: args.func)
    p.set_defaults(func=func)


def build_parser():
    parser = argparse.ArgumentParser(
        description='n-gram text-reuse search of fan works against a script '
                    '(MI355X build of the `ao3.py search` path).')
    subparsers = parser.add_subparsers(help='search, format, matrix, passages, works, quotes, variants, pairs, groups, clusters, readings, retellings, companions, transitions, sources or validate')

    validate_parser = subparsers.add_parser('validate', help='validate script markup')
    validate_parser.add_argument('script', action='store',
                                 help='filename for markup version of script')
    validate_parser.set_defaults(func=_validate)

    search_parser = subparsers.add_parser(
        'search', help='compare fanworks with the original script')
    search_parser.add_argument('fan_works', action='store',
                               help='directory of fanwork text files')
    search_parser.add_argument('script', action=_Scripts, nargs='+', metavar='script',
                               help='filename for markup version of script; with several, every '
                                    'batch of fan works is read once and searched with each script, '
                                    'whose files go to <out-dir>/<script name>/')
    search_parser.add_argument('--out-dir', default=None,
                               help='directory of the batch files and the dated file (default: the '
                                    'working directory; with several scripts a directory per script '
                                    'inside it)')
    search_parser.add_argument('-n', '--num-works', default=-1, type=int,
                               help="number of works to search (for subsampling)")
    search_parser.add_argument('-s', '--skip-works', default=0, type=int,
                               help="number of works to skip (for subsampling)")
    # additions; defaults reproduce the reference's behaviour
    search_parser.add_argument('--window-size', default=None, type=int,
                               help='n-gram size (reference: fixed at 6)')
    search_parser.add_argument('--device', default=0, type=int,
                               help='HIP device ordinal')
    search_parser.add_argument('--vectors', default=None,
                               help="vector table, .npz with 'words' and 'vectors' (what the "
                                    "reference takes from spaCy's en_core_web_md); also "
                                    "FANDOM_SEARCH_VECTORS")
    search_parser.add_argument('--synthetic-vocab', action='store_true',
                               help='use the synthetic benchmark vocabulary (8192 pseudo-words '
                                    'with random vectors: no semantic similarity)')
    search_parser.add_argument('--unique-filter', default=None, type=int, choices=(0, 1),
                               help="NearPy's UniqueFilter on a query's bucket contents: 0 = what "
                                    "NearPy 1.0.0 does for the reference's call (default), 1 = "
                                    "NearPy 0.2.x; also FANDOM_SEARCH_UNIQUE_FILTER")
    search_parser.add_argument('--listing', default=None, choices=('sorted', 'os'),
                               help="order of the directory listing in front of the seeded shuffle: "
                                    "'sorted' (default: a run repeats anywhere) or 'os' (os.listdir() as "
                                    "it comes, what the reference shuffles); also FANDOM_SEARCH_LISTING")
    search_parser.set_defaults(func=_search)

    data_parser = subparsers.add_parser(
        'format', help='takes a script and outputs a csv with reuse counts for each word '
                       'formatted for javascript visualization')
    data_parser.add_argument('matches', action='store', help='filename for search output')
    data_parser.add_argument('script', action='store',
                             help='filename for markup version of script')
    data_parser.add_argument('-o', '--output', action='store', default='js-data.csv',
                             help='filename for csv output file of data formatted for visualization')
    data_parser.add_argument('--lexicon', default=None,
                             help='emotion lexicon, lines "word<TAB>TAG[<TAB>0|1]" '
                                  '(the reference uses lextrie emolex_en)')
    data_parser.add_argument('--device', default=0, type=int, help='HIP device ordinal')
    data_parser.set_defaults(func=_format)

    matrix_parser = subparsers.add_parser(
        'matrix', help='deduplicates and builds matrix for best n-gram matches')
    matrix_parser.add_argument('i', action='store', help='input csv file')
    matrix_parser.add_argument('m', action='store',
                               help='fandom/movie name for output file prefix')
    matrix_parser.add_argument('-n', action='store', default=6, type=int,
                               help='n-gram size, default is 6-grams')
    matrix_parser.add_argument('--engine', default='python', choices=('python', 'device'),
                               help='where the spans are joined, counted and chosen: python '
                                    '(the default, no GPU needed) or device (the GPU; a file it '
                                    'does not take goes to python)')
    matrix_parser.add_argument('--device', default=0, type=int, help='HIP device ordinal')
    matrix_parser.add_argument('--cells', action='store_true',
                               help='also write the matrix without its zeros, one row per '
                                    'non-zero cell, to ...-gram-match-cells.csv')
    matrix_parser.set_defaults(func=_matrix)

    _analysis(subparsers, 'passages',
              'joins the per-word records of a match csv into passages of reuse',
              'filename for the passages csv (default: the input name '
              'with .csv replaced by -passages.csv)',
              [_SPANS])

    _analysis(subparsers, 'works',
              'summarises the records of a match csv by fan work: how much each work '
              'reuses, and from which scenes and characters',
              'prefix of the three csv files, PREFIX-works.csv, '
              'PREFIX-works-scenes.csv and PREFIX-works-characters.csv '
              '(default: the input name without .csv)',
              [_SPANS])

    _analysis(subparsers, 'quotes',
              'ranks the stretches of the script by the fan works that quote them: '
              'per script word and per quoted region, how many works and passages',
              'prefix of the two csv files, PREFIX-quotes.csv and '
              'PREFIX-quotes-words.csv (default: the input name without '
              '.csv)',
              [(lambda a: a.min_words < 1 or a.min_works < 1 or a.max_gap < 0,
                '--min-words and --min-works must be at least 1, --max-gap at least 0')],
              last=[_own('--min-works', default=1, type=int,
                         help='fewest different works whose passages cover every word of '
                              'a region, default 1')])

    _analysis(subparsers, 'variants',
              'ranks, under each script word, the spellings fans wrote there: per '
              'script word and fan spelling, how many records and works',
              'prefix of the two csv files, PREFIX-variants.csv and '
              'PREFIX-variants-words.csv (default: the input name '
              'without .csv)',
              [(lambda a: a.top < 0 or a.min_records < 1,
                '--top must be at least 0, --min-records at least 1')],
              spans=False,
              last=[_own('--top', default=10, type=int,
                         help='spellings listed per script word, the most frequent '
                              'first; 0: all; default 10'),
                    _own('--min-records', default=1, type=int,
                         help='fewest records a listed spelling has, default 1'),
                    _own('--fold-case', action='store_true',
                         help='spellings equal when lower-cased are one spelling, shown '
                              'as its first appearance wrote it')])

    _analysis(subparsers, 'pairs',
              'ranks the pairs of fan works by the script words both quote: per pair '
              'the shared words and their longest run, per work its closest partner',
              'prefix of the two csv files, PREFIX-pairs.csv and '
              'PREFIX-pairs-works.csv (default: the input name without '
              '.csv)',
              [(lambda a: a.min_words < 1 or a.min_shared < 1 or a.max_gap < 0,
                '--min-words and --min-shared must be at least 1, --max-gap at least 0')],
              last=[_own('--min-shared', default=6, type=int,
                         help='fewest script words the passages of both works of a listed '
                              'pair cover, default 6')])

    _analysis(subparsers, 'groups',
              'reduces the reuse by groups of fan works taken from the metadata csv '
              '(year, month, author, language or tag): per group its works, passages '
              'and covered script words, per scene and per script word the works',
              'prefix of the three csv files, PREFIX-groups.csv, '
              'PREFIX-groups-scenes.csv and PREFIX-groups-words.csv '
              '(default: the input name without .csv)',
              [(lambda a: a.min_words < 1 or a.min_works < 1 or a.max_gap < 0,
                '--min-words and --min-works must be at least 1, --max-gap at least 0')],
              first=[_own('meta', action='store',
                          help='filename for the metadata csv (FILENAME, TITLE, AUTHOR, '
                               'SUMMARY, NOTES, PUBLICATION_DATE, LANGUAGE, TAGS)'),
                     _own('--by', default='year',
                          help='what groups the works: year, month, author, language, tag '
                               'or tag:<Category>; default year')],
              last=[_own('--min-works', default=1, type=int,
                         help='fewest works of a group whose passages cover a listed '
                              'script word, default 1')])

    _analysis(subparsers, 'clusters',
              'gathers the fan works quoting the same lines into families (connected '
              'components of the works linked by shared script words): per family '
              'its size, its hub and the words its members have in common, per work '
              'its family',
              'prefix of the two csv files, PREFIX-clusters.csv and '
              'PREFIX-clusters-works.csv (default: the input name '
              'without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_shared < 1 or a.min_size < 1
                           or a.max_gap < 0),
                '--min-words, --min-shared and --min-size must be at least 1, --max-gap at '
                'least 0'),
               (lambda a: not 0 <= a.min_jaccard <= 100 or not 1 <= a.common <= 100,
                '--min-jaccard must be from 0 to 100, --common from 1 to 100')],
              last=[_own('--min-shared', default=6, type=int,
                         help='fewest script words the passages of two linked works '
                              'both cover, default 6'),
                    _own('--min-jaccard', default=50, type=int,
                         help='fewest shared words of two linked works as a whole '
                              'percentage of the words either covers, 0 to 100, '
                              'default 50'),
                    _own('--min-size', default=2, type=int,
                         help='fewest works of a listed family, default 2'),
                    _own('--common', default=50, type=int,
                         help='a script word is common to a family when at least this '
                              'whole percentage of its works cover it, 1 to 100, '
                              'default 50')])

    _analysis(subparsers, 'readings',
              'collates the wordings fans give each quoted stretch of the script: '
              'per span and reading (the fan words of a passage), how many passages '
              'and works',
              'prefix of the two csv files, PREFIX-readings.csv and '
              'PREFIX-readings-spans.csv (default: the input name '
              'without .csv)',
              [(lambda a: a.min_words < 1 or a.min_works < 1 or a.max_gap < 0 or a.top < 0,
                '--min-words and --min-works must be at least 1, --max-gap and --top at '
                'least 0')],
              last=[_own('--top', default=10, type=int,
                         help='readings listed per span, those of the most works '
                              'first; 0: all; default 10'),
                    _own('--min-works', default=1, type=int,
                         help='fewest works a listed reading has, default 1'),
                    _own('--fold-case', action='store_true',
                         help='fan words equal when lower-cased are one spelling')])

    _analysis(subparsers, 'retellings',
              'lists the fan works that quote the script in its order: per work '
              'the heaviest chain of passages that advance through the script as '
              'they advance through the work, and every passage with its place '
              'in the chain',
              'prefix of the two csv files, PREFIX-retellings.csv and '
              'PREFIX-retellings-passages.csv (default: the input name '
              'without .csv)',
              [(lambda a: a.min_words < 1 or a.min_passages < 1 or a.max_gap < 0,
                '--min-words and --min-passages must be at least 1, --max-gap at least 0'),
               _SHARE],
              last=[_own('--min-passages', default=2, type=int,
                         help='fewest passages in the chain of a listed work, '
                              'default 2'),
                    _own('--min-share', default=0, type=int,
                         help='fewest passage words of a listed work that lie in its '
                              'chain, as a whole percentage, 0 to 100, default 0')])

    by_unit = _own('--by', default='region', choices=('region', 'scene', 'character'),
                   help='the units: the quoted regions of `quotes` (default), '
                        'the scenes or the characters of the script')
    region_works = _own('--min-works', default=1, type=int,
                        help='with --by region: fewest different works whose passages '
                             'cover every word of a region, default 1')

    _analysis(subparsers, 'companions',
              'relates the quoted stretches of the script to each other: per pair '
              'of quoted regions, scenes or characters the fan works that quote '
              'both, per unit its closest companion',
              'prefix of the two csv files, PREFIX-companions.csv and '
              'PREFIX-companions-units.csv (default: the input name '
              'without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_both < 1
                           or a.max_gap < 0),
                '--min-words, --min-works and --min-both must be at least 1, --max-gap at '
                'least 0'),
               _SHARE],
              middle=[by_unit],
              last=[region_works,
                    _own('--min-both', default=2, type=int,
                         help='fewest works quoting both units of a listed pair, '
                              'default 2'),
                    _own('--min-share', default=0, type=int,
                         help='fewest works quoting both units as a whole percentage '
                              'of the works of the less quoted one, 0 to 100, default 0')])

    _analysis(subparsers, 'transitions',
              'counts which stretch of the script the fan works quote next: per '
              'pair (from, to) of quoted regions, scenes or characters the steps '
              'from one to the other, per unit its most usual successor',
              'prefix of the two csv files, PREFIX-transitions.csv and '
              'PREFIX-transitions-units.csv (default: the input name '
              'without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_steps < 1
                           or a.min_step_works < 1 or a.max_gap < 0),
                '--min-words, --min-works, --min-steps and --min-step-works must be at least '
                '1, --max-gap at least 0'),
               (lambda a: a.within is not None and not 0 <= a.within < 0xFFFFFFFF,
                '--within must be from 0 to 4294967294 (leave it out for any distance)'),
               _SHARE],
              middle=[by_unit],
              last=[region_works,
                    _own('--within', default=None, type=int,
                         help='most fan words between the two passages of a step, '
                              'default any distance'),
                    _own('--min-steps', default=1, type=int,
                         help='fewest steps of a listed cell, default 1'),
                    _own('--min-step-works', default=2, type=int,
                         help='fewest different works taking the step of a listed '
                              'cell, default 2'),
                    _own('--min-share', default=0, type=int,
                         help='fewest steps of a listed cell as a whole percentage of '
                              'the steps leaving its first unit, 0 to 100, default 0')])

    _analysis(subparsers, 'sources',
              'joins the match files of one corpus searched against several scripts: '
              'which script each fan passage quotes, where passages of different '
              'scripts lie on the same fan words and which of them wins',
              'prefix of the four csv files, PREFIX-sources.csv, '
              'PREFIX-sources-works.csv, PREFIX-sources-scripts.csv and '
              'PREFIX-sources-pairs.csv',
              [_SPANS], several=True,
              middle=[_own('--names', default=None,
                           help="the scripts' names, comma-separated, one per file "
                                "(default: the files' parent directories when they "
                                'differ, else the file names without .csv)')])
    return parser


def full_parser():
    """build_parser(), whose surface tests/golden/cli_surface.json pins as it stands, and behind
    it `alignments`, with a pinned surface of its own (tests/golden/alignments_cli.json) that
    holds this parser to exactly these commands; ao3_parser() goes on from here."""
    parser = build_parser()
    subparsers = parser._subparsers._group_actions[0]
    subparsers.help = subparsers.help.replace(' or validate', ', alignments or validate')

    _analysis(subparsers, 'alignments',
              'aligns every fan work against the script with gaps: quotes with '
              'inserted or dropped words, or a stray record between their halves, '
              'that `passages` breaks in two; per alignment its words, score and '
              'skipped words, per work what it gains over its passages',
              'prefix of the two csv files, PREFIX-alignments.csv and '
              'PREFIX-alignments-works.csv (default: the input name '
              'without .csv)',
              [(lambda a: (a.min_words < 1 or a.match < 1 or not 0 <= a.reach <= 63
                           or not 0 <= a.gap <= 16 or a.match > 16),
                '--min-words and --match must be at least 1, --reach from 0 to 63, --gap '
                'from 0 to 16, --match at most 16')],
              spans=False,
              last=[_own('--min-words', default=6, type=int,
                         help='fewest matched words an alignment has, default 6'),
                    _own('--reach', default=4, type=int,
                         help='most words a link skips on either side, 0 to 63, '
                              'default 4'),
                    _own('--match', default=2, type=int,
                         help='what a matched word scores, 1 to 16, default 2'),
                    _own('--gap', default=1, type=int,
                         help='what a skipped word costs, 0 to 16, default 1')])
    return parser


def ao3_parser():
    """The parser `ao3.py` runs: full_parser(), whose surface the tests pin as it stands, and
    behind it the commands added since (`lines`, `fragments`, `digest`, `intervals`,
    `contrast`, `saturation`, `trends`, `neighbours`, `misquotes`, `tree`, `bundles`,
    `routes`, `fanon`)."""
    parser = full_parser()
    subparsers = parser._subparsers._group_actions[0]
    subparsers.help = subparsers.help.replace(' or validate', ', lines, fragments, digest, intervals, bundles, routes, fanon, trends, neighbours, misquotes, tree, contrast, saturation or validate')

    _analysis(subparsers, 'lines',
              'ranks the lines of the script markup by the fan works quoting them '
              'and says how completely: per line the works quoting it whole, mostly, '
              'from its first word and to its last, per work its lines, per line and '
              'work the covered words',
              'prefix of the three csv files, PREFIX-lines.csv, '
              'PREFIX-lines-works.csv and PREFIX-lines-cells.csv (default: the input '
              'name without .csv)',
              [(lambda a: a.min_words < 1 or a.min_works < 1 or a.max_gap < 0,
                '--min-words and --min-works must be at least 1, --max-gap at least 0'),
               (lambda a: not 1 <= a.most <= 100, '--most must be from 1 to 100')],
              first=[_own('script', action='store',
                          help='filename for the script markup the csv was searched '
                               'against')],
              last=[_own('--min-works', default=1, type=int,
                         help='fewest works quoting a listed line, default 1'),
                    _own('--most', default=50, type=int,
                         help='fewest words of a line, as a whole percentage of its '
                              'words, a work covers to count in MOST_WORKS, 1 to 100, '
                              'default 50')])

    _analysis(subparsers, 'fragments',
              'lists the phrases the fan works quote word for word: every stretch of '
              'the script that --min-works works quote in full and that loses a work '
              'with one more word on either side, a phrase inside a longer quote '
              'included; per work its unbroken runs and the fragments they hold',
              'prefix of the two csv files, PREFIX-fragments.csv and '
              'PREFIX-fragments-works.csv (default: the input name without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_length < 1
                           or a.max_gap < 0 or a.top < 0),
                '--min-words, --min-works and --min-length must be at least 1, --max-gap '
                'and --top at least 0'),
               (lambda a: not a.min_length <= a.max_words <= 4096,
                '--max-words must be from --min-length to 4096')],
              last=[_own('--min-works', default=2, type=int,
                         help='fewest works quoting a listed fragment in full, default 2'),
                    _own('--min-length', default=3, type=int,
                         help='fewest words of a listed fragment, default 3'),
                    _own('--max-words', default=128, type=int,
                         help='most words of a listed fragment, up to 4096, default 128; '
                              'longer ones are not listed, and a stretch of this many '
                              'words that goes on with the same works is none'),
                    _own('--top', default=0, type=int,
                         help='keep the first N fragments of the ranking, default 0: all')])

    _analysis(subparsers, 'digest',
              'picks the fewest fan works that together show what the works quote: '
              'the work covering most of the script first, then always the work that '
              'adds most words to what the picks so far cover; per pick what it adds '
              'and how much of the quoted script the picks cover by then, per work how '
              'much of it the picks show and which pick is most like it',
              'prefix of the two csv files, PREFIX-digest.csv and '
              'PREFIX-digest-works.csv (default: the input name without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_gain < 1 or a.max_gap < 0
                           or a.picks < 0),
                '--min-words and --min-gain must be at least 1, --max-gap and --picks at '
                'least 0'),
               (lambda a: not 1 <= a.cover <= 100, '--cover must be from 1 to 100')],
              last=[_own('--picks', default=0, type=int,
                         help='most works to pick, default 0: no limit'),
                    _own('--cover', default=100, type=int,
                         help='stop once the picks cover this whole percentage of the '
                              'script words any work quotes, 1 to 100, default 100'),
                    _own('--min-gain', default=1, type=int,
                         help='stop when no work adds this many new words, default 1')])

    _analysis(subparsers, 'intervals',
              'says how sure the works-per-stretch counts are: a Poisson bootstrap '
              'over the fan works, per quoted region, script word, scene or character '
              'the interval and median of its works over the replicates, its rank, and '
              'in how many replicates it stays ahead of the next unit; per replicate the '
              'works drawn',
              'prefix of the two csv files, PREFIX-intervals.csv and '
              'PREFIX-intervals-replicates.csv (default: the input name without .csv)',
              [(lambda a: a.min_words < 1 or a.min_works < 1 or a.max_gap < 0,
                '--min-words and --min-works must be at least 1, --max-gap at least 0'),
               (lambda a: not 1 <= a.replicates <= 4096, '--replicates must be from 1 to 4096'),
               (lambda a: not 50 <= a.level <= 99, '--level must be from 50 to 99'),
               (lambda a: not 0 <= a.seed < 1 << 64, '--seed must be from 0 to 2^64 - 1')],
              middle=[_own('--by', default='region',
                           choices=('region', 'word', 'scene', 'character'),
                           help='the units: the quoted regions of `quotes` (default), '
                                'every script word inside one, the scenes or the '
                                'characters of the script')],
              last=[_own('--min-works', default=1, type=int,
                         help='with --by region or word: fewest different works whose '
                              'passages cover every word of a region, default 1'),
                    _own('--replicates', default=1000, type=int,
                         help='resamples of the works, 1 to 4096, default 1000'),
                    _own('--seed', default=0, type=int,
                         help='seed of the multiplicities, 0 to 2^64 - 1, default 0'),
                    _own('--level', default=95, type=int,
                         help='the interval as a whole percentage, 50 to 99, default 95')])

    _analysis(subparsers, 'contrast',
              'says what one group of fan works quotes more than another: two sides taken '
              'from the metadata csv, per quoted region, script word, scene or character the '
              'share of either side quoting it, how often a random relabelling of the works '
              'differs as much, and how often the largest difference over all units does '
              '(a permutation test with the max-statistic correction)',
              'prefix of the three csv files, PREFIX-contrast.csv, PREFIX-contrast-sides.csv '
              'and PREFIX-contrast-permutations.csv (default: the input name without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_quoting < 1
                           or a.max_gap < 0),
                '--min-words, --min-works and --min-quoting must be at least 1, --max-gap at '
                'least 0'),
               (lambda a: not 1 <= a.permutations <= 4096,
                '--permutations must be from 1 to 4096'),
               (lambda a: not 0 <= a.seed < 1 << 64, '--seed must be from 0 to 2^64 - 1')],
              first=[_own('meta', action='store',
                          help='filename for the metadata csv (FILENAME, TITLE, AUTHOR, '
                               'SUMMARY, NOTES, PUBLICATION_DATE, LANGUAGE, TAGS)'),
                     _own('--a', action='append', required=True, metavar='KEY',
                          help='a key of side A; may be given several times'),
                     _own('--b', action='append', default=None, metavar='KEY',
                          help='a key of side B; may be given several times; default: side B '
                               'is every work that does not match --a'),
                     _own('--by', default='year',
                          help='what the keys are: year, month, author, language, tag or '
                               'tag:<Category>; default year')],
              middle=[_own('--unit', default='region',
                           choices=('region', 'word', 'scene', 'character'),
                           help='the units: the quoted regions of `quotes` (default), '
                                'every script word inside one, the scenes or the '
                                'characters of the script')],
              last=[_own('--min-works', default=1, type=int,
                         help='with --unit region or word: fewest different works whose '
                              'passages cover every word of a region, default 1'),
                    _own('--min-quoting', default=5, type=int,
                         help='fewest works of both sides together quoting a unit of the '
                              'family the adjustment covers, default 5'),
                    _own('--permutations', default=1000, type=int,
                         help='relabellings of the works, 1 to 4096, default 1000'),
                    _own('--seed', default=0, type=int,
                         help='seed of the relabellings, 0 to 2^64 - 1, default 0')])

    _analysis(subparsers, 'saturation',
              'says whether the sample of works is large enough: random orders of the fan '
              'works, per point of the curve how many script words inside a quoted region, '
              'regions, scenes or characters a sample of that share of the works has seen, '
              'as an interval, median and mean over the orders beside the sample\'s size; '
              'per order where it passes half, nine tenths and all of them; and the Chao2 '
              'lower bound of what is still unseen',
              'prefix of the three csv files, PREFIX-saturation.csv, '
              'PREFIX-saturation-permutations.csv and PREFIX-saturation-summary.csv '
              '(default: the input name without .csv)',
              [(lambda a: a.min_words < 1 or a.min_works < 1 or a.max_gap < 0,
                '--min-words and --min-works must be at least 1, --max-gap at least 0'),
               (lambda a: not 1 <= a.permutations <= 4096,
                '--permutations must be from 1 to 4096'),
               (lambda a: not 1 <= a.points <= 1024, '--points must be from 1 to 1024'),
               (lambda a: not 50 <= a.level <= 99, '--level must be from 50 to 99'),
               (lambda a: not 0 <= a.seed < 1 << 64, '--seed must be from 0 to 2^64 - 1')],
              middle=[_own('--by', default='word',
                           choices=('region', 'word', 'scene', 'character'),
                           help='the units: every script word inside a quoted region of '
                                '`quotes` (default), the regions, the scenes or the '
                                'characters of the script')],
              last=[_own('--min-works', default=1, type=int,
                         help='with --by region or word: fewest different works whose '
                              'passages cover every word of a region, default 1'),
                    _own('--permutations', default=1000, type=int,
                         help='orders of the works, 1 to 4096, default 1000'),
                    _own('--points', default=100, type=int,
                         help='points of the curve, evenly spaced sample shares, 1 to 1024, '
                              'default 100'),
                    _own('--seed', default=0, type=int,
                         help='seed of the orders, 0 to 2^64 - 1, default 0'),
                    _own('--level', default=95, type=int,
                         help='the interval as a whole percentage, 50 to 99, default 95')])

    _analysis(subparsers, 'trends',
              'says which stretches the later fan works quote more and which the earlier: '
              'every dated work has a period from the metadata csv, per quoted region, script '
              'word, scene or character whether the works quoting it are later or earlier '
              'than the works as a whole, by how much, how often a random re-dating of the '
              'works shifts them as far, and how often the largest shift over all units does '
              '(the max-statistic correction of `contrast`)',
              'prefix of the three csv files, PREFIX-trends.csv, PREFIX-trends-periods.csv '
              'and PREFIX-trends-permutations.csv (default: the input name without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_quoting < 1
                           or a.max_gap < 0),
                '--min-words, --min-works and --min-quoting must be at least 1, --max-gap at '
                'least 0'),
               (lambda a: not 1 <= a.permutations <= 4096,
                '--permutations must be from 1 to 4096'),
               (lambda a: not 0 <= a.seed < 1 << 64, '--seed must be from 0 to 2^64 - 1')],
              first=[_own('meta', action='store',
                          help='filename for the metadata csv (FILENAME, TITLE, AUTHOR, '
                               'SUMMARY, NOTES, PUBLICATION_DATE, LANGUAGE, TAGS)'),
                     _own('--by', default='year',
                          help='the periods: year (default) or month of PUBLICATION_DATE')],
              middle=[_own('--unit', default='region',
                           choices=('region', 'word', 'scene', 'character'),
                           help='the units: the quoted regions of `quotes` (default), '
                                'every script word inside one, the scenes or the '
                                'characters of the script')],
              last=[_own('--min-works', default=1, type=int,
                         help='with --unit region or word: fewest different works whose '
                              'passages cover every word of a region, default 1'),
                    _own('--min-quoting', default=5, type=int,
                         help='fewest dated works quoting a unit of the family the '
                              'adjustment covers, default 5'),
                    _own('--permutations', default=1000, type=int,
                         help='re-datings of the works, 1 to 4096, default 1000'),
                    _own('--seed', default=0, type=int,
                         help='seed of the re-datings, 0 to 2^64 - 1, default 0')])

    _analysis(subparsers, 'neighbours',
              'lists each fan work\'s closest works by the rare lines both quote: a script '
              'word weighs the more the fewer works cover it, the similarity of two works is '
              'the weighted Jaccard of their coverages in parts per million; per work its '
              '--top closest works with the rarest word they share and the run around it, '
              'per work how its list and the others\' hold each other, per script word its '
              'depth and weight',
              'prefix of the three csv files, PREFIX-neighbours.csv, '
              'PREFIX-neighbours-works.csv and PREFIX-neighbours-words.csv (default: the '
              'input name without .csv)',
              [(lambda a: not 1 <= a.top <= 32, '--top must be from 1 to 32'),
               (lambda a: a.min_score < 1, '--min-score must be at least 1'),
               (lambda a: not 0 <= a.min_similarity <= 100,
                '--min-similarity must be from 0 to 100'),
               _SPANS],
              middle=[_own('--weight', default='rarity', choices=('rarity', 'flat'),
                           help='what a shared script word weighs: the bits of (active works '
                                '// works covering it), 1 for a word more than half the '
                                'works cover (rarity, default), or 1 (flat)'),
                      _own('--top', default=10, type=int,
                           help='most neighbours listed per work, 1 to 32, default 10'),
                      _own('--min-score', default=1, type=int,
                           help='smallest weighted sum of the shared words of a candidate, '
                                'default 1'),
                      _own('--min-similarity', default=0, type=int,
                           help='smallest similarity of a candidate as a whole percentage, '
                                '0 to 100, default 0')])

    _analysis(subparsers, 'misquotes',
              'lists the works that share departures from the script: a misquote is a '
              'script word with a fan spelling that is not its own, inside a passage; one '
              'that few of the works quoting the word share is telling and weighs the more '
              'the fewer share it; per listed misquote its records, works and readers, per '
              'pair of works the telling misquotes both have, their score and how much of '
              'their common ground they agree on, per work its departures and its closest '
              'work',
              'prefix of the three csv files, PREFIX-misquotes.csv, '
              'PREFIX-misquotes-pairs.csv and PREFIX-misquotes-works.csv (default: the '
              'input name without .csv)',
              [(lambda a: a.min_works < 2, '--min-works must be at least 2'),
               (lambda a: not 1 <= a.max_share <= 100, '--max-share must be from 1 to 100'),
               (lambda a: a.min_shared < 1 or a.min_score < 1,
                '--min-shared and --min-score must be at least 1'),
               _SPANS],
              last=[_own('--min-works', default=2, type=int,
                         help='fewest different works a listed misquote has, at least 2, '
                              'default 2'),
                    _own('--max-share', default=50, type=int,
                         help='most of the works quoting a script word, as a whole '
                              'percentage, that may share a telling misquote of it, 1 to '
                              '100, default 50'),
                    _own('--weight', default='rarity', choices=('rarity', 'flat'),
                         help='what a telling misquote weighs: the bits of (works quoting '
                              'the word // works sharing the misquote) (rarity, default), '
                              'or 1 (flat)'),
                    _own('--min-shared', default=1, type=int,
                         help='fewest telling misquotes a kept pair shares, default 1'),
                    _own('--min-score', default=1, type=int,
                         help='smallest sum of their weights of a kept pair, default 1'),
                    _own('--keep-case', action='store_true',
                         help='compare the fan words with the script as written; by '
                              'default spellings equal in lower case are one')])

    _analysis(subparsers, 'tree',
              'shows how the families of `clusters` merge as the bar drops, every bar at '
              'once: two works sharing --min-shared script words have an edge at the level '
              'of their Jaccard in parts per million (or of their shared words), the edges '
              'are taken from the highest level down and one between two families merges '
              'them; per merge its level, its edge and the two sides, per work its tree, '
              'its first merge and its place in a leaf order, per level the families there '
              'are then',
              'prefix of the three csv files, PREFIX-tree.csv, PREFIX-tree-works.csv and '
              'PREFIX-tree-levels.csv (default: the input name without .csv)',
              [(lambda a: a.min_shared < 1, '--min-shared must be at least 1'),
               (lambda a: a.min_level < 0 or (a.measure == 'jaccard' and a.min_level > 1000000),
                '--min-level must be at least 0, and at most 1000000 under --measure jaccard'),
               (lambda a: a.min_level > 0xFFFFFFFF, '--min-level must be below 2^32'),
               _SPANS],
              middle=[_own('--measure', default='jaccard', choices=('jaccard', 'shared'),
                           help='the level of an edge: the shared words as parts per million '
                                'of the words either work covers, rounded down (jaccard, '
                                'default), or the shared words (shared)'),
                      _own('--min-shared', default=6, type=int,
                           help='fewest script words two works share to have an edge, '
                                'default 6'),
                      _own('--min-level', default=0, type=int,
                           help='smallest level of an edge, default 0')])

    _analysis(subparsers, 'bundles',
              'lists the sets of quoted regions, scenes or characters that the same '
              'fan works quote: every set of 2 to --max-size units that at least '
              '--min-all works quote in full, whether it is closed, the sets '
              'extending it, per unit the sets holding it, per size the counts',
              'prefix of the three csv files, PREFIX-bundles.csv, '
              'PREFIX-bundles-units.csv and PREFIX-bundles-levels.csv (default: the '
              'input name without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_all < 1
                           or a.max_gap < 0),
                '--min-words, --min-works and --min-all must be at least 1, --max-gap at '
                'least 0'),
               (lambda a: not 2 <= a.max_size <= 8, '--max-size must be from 2 to 8')],
              middle=[_own('--by', default='region', choices=('region', 'scene', 'character'),
                           help='the units: the quoted regions of `quotes` (default), '
                                'the scenes or the characters of the script')],
              last=[_own('--min-works', default=1, type=int,
                         help='with --by region: fewest different works whose passages '
                              'cover every word of a region, default 1'),
                    _own('--min-all', default=5, type=int,
                         help='fewest works quoting every unit of a set, default 5'),
                    _own('--max-size', default=4, type=int,
                         help='most units in a listed set, 2 to 8, default 4; the sets '
                              'of one unit more are mined too and not listed'),
                    _own('--all', action='store_true',
                         help='list every frequent set, not only the closed ones')])

    _analysis(subparsers, 'routes',
              'lists the sequences of quoted regions, scenes or characters that the '
              'fan works quote in that order: every route of 2 to --max-length units '
              'that at least --min-all works follow, whether it is closed, the routes '
              'continuing it, per unit the routes holding it, per length the counts',
              'prefix of the three csv files, PREFIX-routes.csv, '
              'PREFIX-routes-units.csv and PREFIX-routes-levels.csv (default: the '
              'input name without .csv)',
              [(lambda a: (a.min_words < 1 or a.min_works < 1 or a.min_all < 1
                           or a.max_gap < 0),
                '--min-words, --min-works and --min-all must be at least 1, --max-gap at '
                'least 0'),
               (lambda a: not 2 <= a.max_length <= 8, '--max-length must be from 2 to 8'),
               (lambda a: a.max_skip is not None and not 0 <= a.max_skip <= 63,
                '--max-skip must be from 0 to 63')],
              middle=[_own('--by', default='region', choices=('region', 'scene', 'character'),
                           help='the units: the quoted regions of `quotes` (default), '
                                'the scenes or the characters of the script')],
              last=[_own('--min-works', default=1, type=int,
                         help='with --by region: fewest different works whose passages '
                              'cover every word of a region, default 1'),
                    _own('--min-all', default=5, type=int,
                         help='fewest works following a route, default 5'),
                    _own('--max-length', default=4, type=int,
                         help='most units in a listed route, 2 to 8, default 4; the '
                              'routes of one unit more are mined too and not listed'),
                    _own('--max-skip', default=None, type=int,
                         help='most other elements of a work\'s sequence between two '
                              'units of a route, 0 to 63; 0: the route is a contiguous '
                              'run; default: any distance'),
                    _own('--all', action='store_true',
                         help='list every frequent route, not only the closed ones')])

    _fanon_parser(subparsers)
    return parser


FANON_CHECKS = [
    (lambda a: not 2 <= a.length <= 32, '--length must be from 2 to 32'),
    (lambda a: a.min_works < 1, '--min-works must be at least 1'),
    (lambda a: not 1 <= a.max_share <= 100, '--max-share must be from 1 to 100'),
    (lambda a: a.top < 0, '--top must be at least 0')]


def _fanon_parser(subparsers):
    """`fanon`, the one analysis command over the fan works themselves and no match csv: its
    arguments are those `search` lists the works with, and its own."""
    p = subparsers.add_parser(
        'fanon', help='lists the phrases fan works share with each other and the script '
                      'lacks: runs of --length-token grams that at least --min-works works '
                      'hold, no script holds and not more than --max-share percent of the '
                      'works hold; per work how much of it is shared, and its longest '
                      'shared passage')
    p.add_argument('fan_works', action='store', help='directory of fanwork text files')
    p.add_argument('scripts', action='store', nargs='*', metavar='script',
                   help='filenames for markup versions of scripts: a gram that stands in '
                        'one of them is canon and not listed')
    p.add_argument('-o', '--output', action='store', default=None,
                   help='prefix of the four csv files, PREFIX-fanon.csv, '
                        'PREFIX-fanon-passages.csv, PREFIX-fanon-grams.csv and '
                        'PREFIX-fanon-works.csv (default: the base name of the directory)')
    p.add_argument('--length', default=8, type=int,
                   help='tokens of a gram, 2 to 32, default 8')
    p.add_argument('--min-works', default=2, type=int,
                   help='fewest different works holding a shared gram, default 2')
    p.add_argument('--max-share', default=100, type=int,
                   help='a gram that more than this percentage of the listed works hold is '
                        'common (disclaimers, site boilerplate) and not shared, 1 to 100, '
                        'default 100: none is')
    p.add_argument('--keep-case', action='store_true',
                   help='compare the tokens as written instead of under str.lower()')
    p.add_argument('--top', default=1000, type=int,
                   help='keep the first N phrases and grams of their rankings, default '
                        '1000; 0: all')
    p.add_argument('-n', '--num-works', default=-1, type=int,
                   help='number of works to read (for subsampling)')
    p.add_argument('-s', '--skip-works', default=0, type=int,
                   help='number of works to skip (for subsampling)')
    p.add_argument('--listing', default=None, choices=('sorted', 'os'),
                   help="order of the directory listing in front of the seeded shuffle, as for "
                        "`search`; also FANDOM_SEARCH_LISTING")
    p.add_argument('--device', default=0, type=int, help='HIP device ordinal')

    def func(args):
        return _command('fanon', FANON_CHECKS, args)
    func.__name__ = '_fanon'
    p.set_defaults(func=func)


def _validate(args):
    from . import search
    return search.validate_cmd(args)


def _search(args):
    import os
    from . import search
    if getattr(args, 'vectors', None):
        os.environ['FANDOM_SEARCH_VECTORS'] = args.vectors
    if getattr(args, 'synthetic_vocab', False):
        os.environ['FANDOM_SEARCH_SYNTHETIC_VOCAB'] = '1'
    if getattr(args, 'unique_filter', None) is not None:
        os.environ['FANDOM_SEARCH_UNIQUE_FILTER'] = str(args.unique_filter)
    if getattr(args, 'listing', None):
        os.environ['FANDOM_SEARCH_LISTING'] = args.listing
    try:
        search.check_scripts(args)          # (before the library loads or a work is read)
    except ValueError as e:
        sys.exit('ao3.py search: error: %s' % e)
    return search.analyze(args)


def _format(args):
    from . import format as format_mod
    return format_mod.format_data(args)


def _matrix(args):
    from . import matrix
    return matrix.process(args)


def _command(name, checks, args):
    """Runs the analysis command `name` (its module's process): the first of `checks`, pairs
    (condition on args, message), that holds ends it with `ao3.py NAME: error: message`, and
    so does a ValueError of the command."""
    import importlib
    for fails, message in checks:
        if fails(args):
            sys.exit('ao3.py %s: error: %s' % (name, message))
    module = importlib.import_module('.' + name, __package__)
    try:
        if name == 'groups':
            module.check_by(args.by)
        return module.process(args)
    except ValueError as e:
        sys.exit('ao3.py %s: error: %s' % (name, e))


def main(argv=None):
    parser = ao3_parser()
    args = parser.parse_args(argv)
    if hasattr(args, 'func'):
        args.func(args)
    else:
        parser.print_help()
    return 0


if __name__ == '__main__':
    sys.exit(main())
