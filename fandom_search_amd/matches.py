"""The match CSV read on the GPU: what `passages`, `works` and `quotes` start from.

`MatchFile` hands the file's bytes to fs_matches_open (csrc/fs_matches.hip), which splits rows
and fields, converts the five numeric columns and flags the rows whose FAN_WORK_FILENAME
differs from the row in front.  The host numbers the works from those head rows alone, checks
the (work, fan_ix) order and decodes only the fields an output row shows (`text`); `intern`
numbers the spellings of a text column on the device (fs_matches_intern), for `variants`.  The columns
come back in passages.sort_records' form; that function and passages.read_matches stay the
`python` reader and this one's oracle.

The reader does not guess: a file outside its grammar (include/fandom_search.h) leaves
`outside` set and the caller goes through the Python functions, so every odd file and every
error behaves as it always did.  Malformed UTF-8 is such a case (the kernel that classifies the
bytes checks it), and open(..., encoding='utf-8') then raises its UnicodeDecodeError.
"""

import ctypes as C
import os
import time

import numpy as np

from . import _lib, abi
from .passages import _COMB, _DIST, _FNAME

READERS = ('device', 'python')
READER_ENV = 'FANDOM_SEARCH_READER'


def reader_of(args):
    """'device' or 'python': args.reader, else FANDOM_SEARCH_READER, else 'device'."""
    r = getattr(args, 'reader', None) or os.environ.get(READER_ENV, '').strip() or 'device'
    if r not in READERS:
        raise ValueError("reader must be one of %s, not %r" % (', '.join(READERS), r))
    return r


def parse_double(text):
    """(status, value) of the conversion the kernel applies to a distance field, on the host
    (fs_matches_parse_double): abi.FS_DEC_SURE and float(text), or abi.FS_DEC_NOT_MINE and None."""
    raw = text if isinstance(text, bytes) else text.encode('utf-8')
    out = C.c_double(0.0)
    rc = _lib.load().fs_matches_parse_double(raw, len(raw), C.byref(out))
    return rc, (out.value if rc == abi.FS_DEC_SURE else None)


def _device_read(data, device):
    """(info, fan, orig, lev, dist, comb, ix, deferred, handle) of the bytes `data`."""
    L = _lib.load()
    info = abi.FsMatchesInfo()
    h = C.c_void_p()
    _lib.check(L.fs_matches_open(int(device), data.ctypes.data_as(C.c_void_p), len(data),
                                 C.byref(h), C.byref(info)), "fs_matches_open")
    n, nd = int(info.n_rows), int(info.n_deferred)
    fan, orig, lev = (np.empty(n, dtype=np.uint32) for _ in range(3))
    dist, comb = (np.empty(n, dtype=np.float64) for _ in range(2))
    ix = np.empty(n, dtype=abi.MATCH_IX_DTYPE)
    deferred = np.empty(nd, dtype=abi.MATCH_DEFER_DTYPE)
    if info.status != abi.FS_MATCHES_OUTSIDE:
        rc = L.fs_matches_read(h, abi.ptr(fan, C.c_uint32), abi.ptr(orig, C.c_uint32),
                               abi.ptr(lev, C.c_uint32), abi.ptr(dist, C.c_double),
                               abi.ptr(comb, C.c_double), ix.ctypes.data_as(C.c_void_p), n,
                               deferred.ctypes.data_as(C.c_void_p), nd)
        if rc != abi.FS_OK:
            L.fs_matches_close(h)
            _lib.check(rc, "fs_matches_read")
    return info, fan, orig, lev, dist, comb, ix, deferred, h


class MatchFile:
    """A match CSV (a dated file with its header row, or a batch file without) read on HIP
    device `device`.  `outside`: the file is not of the reader's grammar and nothing else of
    the object is of use.  Otherwise: n, status, n_deferred, has_header, names (the works in
    first-appearance order), the columns in file order (work, fan, orig, lev, dist, comb),
    sorted() and text().  `times`: seconds spent reading, on the device call, numbering."""

    def __init__(self, path, device=0):
        t0 = time.perf_counter()
        self.data = np.fromfile(path, dtype=np.uint8)
        t1 = time.perf_counter()
        (info, self.fan, self.orig, self.lev, self.dist, self.comb, self.ix, deferred,
         self._h) = _device_read(self.data, device)
        t2 = time.perf_counter()
        self.status, self.reason = int(info.status), int(info.reason)
        self.has_header = bool(info.has_header)
        self.n, self.n_deferred = int(info.n_rows), int(info.n_deferred)
        self.device_ms = dict(zip(abi.MATCHES_MS_NAMES, info.ms))
        self.outside = self.status == abi.FS_MATCHES_OUTSIDE
        self.names, self.work, self._order = [], np.zeros(0, dtype=np.int64), None
        if not self.outside:
            self._apply(deferred)
        if not self.outside:
            self._number_works()
        self.times = {'read': t1 - t0, 'device': t2 - t1, 'host': time.perf_counter() - t2}

    def close(self):
        if self._h:
            _lib.load().fs_matches_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _apply(self, deferred):
        """float() over the fields the kernel left alone; one that float() refuses makes the
        file the Python reader's, which raises what it always raised."""
        for row, col in zip(deferred['row'].tolist(), deferred['col'].tolist()):
            try:
                value = float(self.text(col, [row])[0])
            except ValueError:
                self.outside = True
                return
            (self.dist if col == _DIST else self.comb)[row] = value
        assert all(c in (_DIST, _COMB) for c in deferred['col'].tolist())

    def _number_works(self):
        heads = np.flatnonzero(self.ix['head'])
        ids, of_head = {}, np.empty(len(heads), dtype=np.int64)
        for k, name in enumerate(self.text(_FNAME, heads)):
            of_head[k] = ids.setdefault(name, len(ids))
        self.names = list(ids)
        self.work = of_head[np.cumsum(self.ix['head'], dtype=np.int64) - 1] if self.n else \
            np.zeros(0, dtype=np.int64)

    def order(self):
        """The stable (work, fan_ix) order of the records: the identity when they lie so."""
        if self._order is None:
            w, f = self.work, self.fan
            if self.n < 2 or bool(np.all((w[1:] > w[:-1]) | ((w[1:] == w[:-1]) & (f[1:] >= f[:-1])))):
                self._order = np.arange(self.n, dtype=np.int64)
            else:
                self._order = np.lexsort((f, w))
        return self._order

    def sorted(self):
        """(order, work, fan_ix, orig_ix, dist, comb) as passages.sort_records gives them."""
        o = self.order()
        return (o, self.work[o], self.fan.astype(np.int64)[o], self.orig.astype(np.int64)[o],
                self.dist[o], self.comb[o])

    def bounds(self, column, records):
        """(first byte, end, quoted) of field `column` of the records."""
        rec = np.asarray(records, dtype=np.int64)
        ix = self.ix[rec]
        start = ix['start'].astype(np.int64)
        a = start + (ix['end'][:, column - 1].astype(np.int64) + 1 if column else 0)
        b = start + ix['end'][:, column].astype(np.int64)
        return a, b, (ix['quoted'] >> np.uint32(column)) & 1 != 0

    def text(self, column, records):
        """The field `column` of the records as csv.reader gives it (a quoted field without
        its quotes, "" as "), decoding nothing else."""
        a, b, quoted = self.bounds(column, records)
        n = len(a)
        if n == 0:
            return []
        lens = np.where(quoted, 0, b - a)
        # the unquoted fields (they hold no line break) gathered behind one another, a '\n'
        # after each, decoded at once
        ends = np.cumsum(lens + 1)
        src = np.repeat(a - (ends - lens - 1), lens + 1) + np.arange(ends[-1], dtype=np.int64)
        buf = self.data[np.minimum(src, len(self.data) - 1)]
        buf[ends - 1] = 10
        out = buf.tobytes().decode('utf-8').split('\n')[:n]
        data = self.data
        for k in np.flatnonzero(quoted).tolist():
            out[k] = data[a[k] + 1:b[k] - 1].tobytes().replace(b'""', b'"').decode('utf-8')
        return out

    def intern(self, column):
        """(id, first) of fs_matches_intern: per record the number of its field's spelling (the
        bytes as written), in first-appearance order, and the first record of every spelling.
        `intern_ms`: the call's HIP-event times."""
        L = _lib.load()
        ids = np.empty(self.n, dtype=np.uint32)
        first = np.empty(self.n, dtype=np.uint32)            # a spelling has a record
        got = C.c_uint64(0)
        _lib.check(L.fs_matches_intern(self._h, int(column), abi.ptr(ids, C.c_uint32),
                                       abi.ptr(first, C.c_uint32), self.n, C.byref(got)),
                   "fs_matches_intern")
        ms = (C.c_double * 8)()
        _lib.check(L.fs_matches_intern_times(self._h, ms), "fs_matches_intern_times")
        self.intern_ms = dict(zip(abi.INTERN_MS_NAMES, ms))
        return ids, first[:got.value]

    def label_rows(self, column, n_script):
        """(first, n_differ) of fs_matches_labels: per script word the smallest record that
        names it (abi.FS_NONE: none), and the records whose field `column` is spelt otherwise
        than that record's."""
        first = np.empty(int(n_script), dtype=np.uint32)
        differ = C.c_uint64(0)
        _lib.check(_lib.load().fs_matches_labels(self._h, int(column), int(n_script),
                                                 abi.ptr(first, C.c_uint32), C.byref(differ)),
                   "fs_matches_labels")
        return first, int(differ.value)

    def labels(self, column, n_script):
        """{script word: text of `column`} over the words with a record, or None when a word's
        records spell the column in two ways (the Python reader then says what is wrong)."""
        first, differ = self.label_rows(column, n_script)
        if differ:
            return None
        words = np.flatnonzero(first != abi.FS_NONE)
        return dict(zip(words.tolist(), self.text(column, first[words])))
