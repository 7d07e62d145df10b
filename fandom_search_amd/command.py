"""The host steps the analysis commands share: the output buffer that grows until the library's
answer fits, the labels of the script's words, the names of the files a command writes, and
the choice of reader with its fallback.  Plain functions: a command's module keeps its own
find_*, tables, tables_device and process and calls these."""

import csv
import ctypes as C

import numpy as np

from . import _lib, abi


def grow(call, dtype, cap, where='library call'):
    """The records a library call writes into a buffer of `cap` records of `dtype`:
    call(buffer, cap, byref(count)) gives the library's code, and on FS_E_CAPACITY the call
    is repeated with room for the count it reported; any other failure is an FsError naming
    `where`.  With a list of dtypes (and of caps) call takes one such triple per
    buffer, in turn, and the arrays come back as a tuple; a buffer that was large enough keeps
    its size."""
    many = isinstance(dtype, (list, tuple))
    dtypes, caps = (list(dtype), list(cap)) if many else ([dtype], [cap])
    while True:
        outs = [np.empty(int(c), dtype=d) for c, d in zip(caps, dtypes)]
        gots = [C.c_uint64(0) for _ in outs]
        triples = [(o.ctypes.data_as(C.c_void_p), int(c), C.byref(g))
                   for o, c, g in zip(outs, caps, gots)]
        rc = call(*[v for t in triples for v in t])
        if rc == abi.FS_E_CAPACITY:
            caps = [max(c, int(g.value)) if many else int(g.value) for c, g in zip(caps, gots)]
            continue
        _lib.check(rc, where)
        found = tuple(o[:g.value] for o, g in zip(outs, gots))
        return found if many else found[0]


def n_script_of(orig):
    """The script's length as the records know it: one past the largest script word index."""
    return int(orig.max()) + 1 if len(orig) else 0


def work_names(rows):
    """The fan works of the records `rows` (read_matches) in first-appearance order."""
    from .passages import _FNAME
    return list(dict.fromkeys(r[_FNAME] for r in rows))


def script_labels(mf, n_script):
    """{script word index: (word, character, scene)} of a matches.MatchFile, each label decoded
    once per script word; None when a script word's records spell one in two ways."""
    from .passages import _CHAR, _ORIG_WORD, _SCENE
    cols = [mf.labels(c, n_script) for c in (_ORIG_WORD, _CHAR, _SCENE)]
    if any(c is None for c in cols):
        return None
    return {o: (w, cols[1][o], cols[2][o]) for o, w in cols[0].items()}


def prefixed(matches, prefix, suffixes):
    """The files a command writes: `prefix` (default: `matches` without its .csv) in front of
    every suffix."""
    if prefix is None:
        prefix = matches[:-4] if matches.endswith('.csv') else matches
    return tuple(prefix + s for s in suffixes)


def write_tables(paths, heads, tables):
    """One CSV per path: its header row, then its table's rows."""
    for path, head, rows in zip(paths, heads, tables):
        with open(path, 'w', newline='', encoding='utf-8') as fh:
            w = csv.writer(fh)
            w.writerow(head)
            w.writerows(rows)


def run(args, heads, outs, tables, tables_device, opts):
    """A command over args.matches: tables_device(mf, *opts) under the device reader,
    tables(rows, *opts) under the python reader, for a file the device reader does not take
    and when tables_device gives None; the tables go to `outs` under `heads`.  Returns
    `outs`."""
    from .matches import MatchFile, reader_of
    from .passages import read_matches
    body = None
    if reader_of(args) == 'device':
        with MatchFile(args.matches, args.device) as mf:
            if not mf.outside:
                body = tables_device(mf, *opts)
    if body is None:
        body = tables(read_matches(args.matches), *opts)
    write_tables(outs, heads, body)
    return outs
