#!/usr/bin/env python3
"""The command line's surface as build_parser() gives it: per sub-command, in the order they
are added, its help and every action in order (option strings, dest, default, type name,
choices, nargs, required, help).  tests/test_command_host.py rebuilds the same structure and
compares it with cli_surface.json, so that a change of cli.py that moves, renames or rewords
an argument shows.

Run from the repo root, on the commit whose surface is to be kept:
  python tests/golden/make_cli_surface.py
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def surface(parser):
    """[[sub-command, its help, [action, ...]], ...] of cli.build_parser()'s parser."""
    sub = parser._subparsers._group_actions[0]
    helps = {a.dest: a.help for a in sub._choices_actions}
    out = []
    for name, p in sub.choices.items():
        actions = [{'option_strings': list(a.option_strings), 'dest': a.dest,
                    'default': a.default,
                    'type': None if a.type is None else a.type.__name__,
                    'choices': None if a.choices is None else list(a.choices),
                    'nargs': a.nargs, 'required': a.required, 'help': a.help}
                   for a in p._actions]
        out.append([name, helps[name], actions])
    return out


if __name__ == '__main__':
    from fandom_search_amd.cli import build_parser
    with open(os.path.join(HERE, 'cli_surface.json'), 'w', encoding='utf-8') as fh:
        json.dump(surface(build_parser()), fh, indent=1)
        fh.write('\n')
