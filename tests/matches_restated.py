"""The grammar of the device match reader (fs_matches_open in include/fandom_search.h, DESIGN.md
section 10) restated as one walk over the file's bytes in plain Python: no tiles, no lanes, no
carried parity.  The oracle of tests/test_matches_restated_host.py, which pins it to
csv.reader and bytes.decode, and of tests/test_gpu_matches_edges.py.  The product never imports
it, and it imports nothing of the product.

The rule, as the header words it:
  * a '"' toggles quoting, ',' outside quotes ends a field, '\\n' outside quotes ends a row, a
    '\\r' directly in front of that '\\n' belongs to the terminator, a last row needs none;
  * over the whole file: no NUL; a quote that opens starts a field (or follows a closing quote:
    the second quote of a "" pair); a quote that closes is followed by ',', '\\n', '\\r', '"' or
    the end of the file (a '\\r' there then falls under the rule for '\\r'); the file does not
    end inside quotes; no '\\r' outside quotes without its '\\n'; the bytes are UTF-8.  The
    reason of a file that breaks any of these is the union of what it breaks, and nothing else
    is looked at;
  * otherwise every non-empty row but a header row (the first non-empty row, byte for byte) is
    a record, and the first of these that fails counts for it: shorter than 2^32 bytes, twelve
    fields, fan_ix / orig_ix / lev unquoted runs of 1..10 digits below 2^32; the reason is the
    union over the records;
  * otherwise a distance field outside fs_dec.h's documented grammar is deferred, and more
    than max(4096, n_rows // 16) of them make the file outside with FS_MATCH_BAD_DEFER alone.
"""

import re

import numpy as np

PARSED, DEFERRED, OUTSIDE = 0, 1, 2
BAD_NUL, BAD_OPEN, BAD_CLOSE, BAD_CR, BAD_FIELDS, BAD_INT, BAD_UTF8, BAD_ROW, BAD_DEFER = \
    1, 2, 4, 8, 16, 32, 64, 128, 256
BYTE_BITS = BAD_NUL | BAD_OPEN | BAD_CLOSE | BAD_CR | BAD_UTF8

FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_INDEX', 'FAN_WORK_WORD', 'FAN_WORK_ORTH_ID',
          'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_ORTH_ID',
          'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'BEST_MATCH_DISTANCE',
          'BEST_LEVENSHTEIN_DISTANCE', 'BEST_COMBINED_DISTANCE']
HEADER = ','.join(FIELDS).encode()
N_FIELDS = 12
INT_COLUMNS = (1, 4, 10)
DISTANCE_COLUMNS = (9, 11)

# fs_dec.h's header comment: "", "nan", "inf", "-inf", or
#   [-] digits [. digits] [(e|E) [+|-] digits]   with at most 17 significant digits
# (leading zeros do not count, trailing ones do)
DECIMAL = re.compile(rb'-?([0-9]+)(?:\.([0-9]+))?(?:[eE][+-]?[0-9]+)?')
INTEGER = re.compile(rb'[0-9]{1,10}')
_SPECIAL = re.compile(rb'[",\r\n\x00]')
_HIGH = re.compile(rb'[\x80-\xff]+')

# first byte -> (continuation bytes, lowest and highest second byte): the well-formed
# sequences of the Unicode standard's table 3-7
_UTF8 = {}
for _c in range(0xC2, 0xE0):
    _UTF8[_c] = (1, 0x80, 0xBF)
for _c in range(0xE0, 0xF0):
    _UTF8[_c] = (2, 0xA0 if _c == 0xE0 else 0x80, 0x9F if _c == 0xED else 0xBF)
for _c in range(0xF0, 0xF5):
    _UTF8[_c] = (3, 0x90 if _c == 0xF0 else 0x80, 0x8F if _c == 0xF4 else 0xBF)


def distance_is_plain(raw):
    """The bytes of a distance field, quotes and all, are of the grammar the device converts."""
    if raw in (b'', b'nan', b'inf', b'-inf'):
        return True
    m = DECIMAL.fullmatch(raw)
    return bool(m) and len((m.group(1) + (m.group(2) or b'')).lstrip(b'0')) <= 17


def utf8_ok(data):
    for m in _HIGH.finditer(data):
        run, i = m.group(), 0
        while i < len(run):
            need, lo, hi = _UTF8.get(run[i], (0, 0, 0))
            if need == 0 or i + need >= len(run):      # (a continuation byte is a high byte)
                return False
            if not lo <= run[i + 1] <= hi:
                return False
            if any(not 0x80 <= b <= 0xBF for b in run[i + 2:i + 1 + need]):
                return False
            i += 1 + need
    return True


def walk(data):
    """(byte-level reason bits without the UTF-8 one, [(start, end, [raw field, ...]), ...] of
    the non-empty rows) under the toggle rule."""
    n, bad, q = len(data), 0, False
    rows, fields = [], []
    row_start = field_start = 0
    closed = -2                                    # where the last closing quote stands
    for m in _SPECIAL.finditer(data):              # (no other byte changes anything)
        i = m.start()
        c = data[i]
        nxt = data[i + 1] if i + 1 < n else -1
        if c == 0:
            bad |= BAD_NUL
        elif c == 0x22:
            if q:
                if nxt not in (-1, 0x2C, 0x0A, 0x0D, 0x22):
                    bad |= BAD_CLOSE
                closed = i
            elif i != field_start and closed != i - 1:
                bad |= BAD_OPEN
            q = not q
        elif q:
            continue
        elif c == 0x2C:
            fields.append(data[field_start:i])
            field_start = i + 1
        elif c == 0x0D:
            if nxt != 0x0A:
                bad |= BAD_CR
        else:
            end = i - 1 if i > field_start and data[i - 1] == 0x0D else i
            if end > row_start:
                fields.append(data[field_start:end])
                rows.append((row_start, end, fields))
            fields = []
            row_start = field_start = i + 1
    if q:
        bad |= BAD_CLOSE
    if row_start < n:
        fields.append(data[field_start:n])
        rows.append((row_start, n, fields))
    return bad, rows


def records_of(data):
    """(byte-level reason, has_header, records): the rows of walk() without the header row."""
    bad, rows = walk(data)
    if not utf8_ok(data):
        bad |= BAD_UTF8
    header = bool(rows) and data[rows[0][0]:rows[0][1]] == HEADER
    return bad, header, rows[1:] if header else rows


def record_reason(start, end, fields):
    if end - start >= 1 << 32:
        return BAD_ROW
    if len(fields) != N_FIELDS:
        return BAD_FIELDS
    for col in INT_COLUMNS:
        if not INTEGER.fullmatch(fields[col]) or int(fields[col]) >= 1 << 32:
            return BAD_INT
    return 0


def deferred_of(records):
    """[(record, column), ...] of the distance fields left to the host."""
    return [(r, col) for r, (_, _, f) in enumerate(records) for col in DISTANCE_COLUMNS
            if not distance_is_plain(f[col])]


def verdict(data):
    """(outside, reason, has_header, n_rows, n_deferred) of the file `data` (bytes)."""
    data = bytes(data)
    bad, header, records = records_of(data)
    if bad:
        return True, bad, False, 0, 0
    for rec in records:
        bad |= record_reason(*rec)
    if bad:
        return True, bad, header, 0, 0
    n_deferred = len(deferred_of(records))
    if n_deferred > max(4096, len(records) // 16):
        return True, BAD_DEFER, header, len(records), n_deferred
    return False, 0, header, len(records), n_deferred


def status_of(v):
    return OUTSIDE if v[0] else DEFERRED if v[4] else PARSED


def field_text(raw):
    """A field as csv.reader gives it: a quoted one without its quotes, "" as "."""
    if raw[:1] == b'"':
        raw = raw[1:-1].replace(b'""', b'"')
    return raw.decode('utf-8')


def text_rows(data):
    """The records of a file inside the grammar as rows of text."""
    return [[field_text(f) for f in fields] for _, _, fields in records_of(bytes(data))[2]]


def field_ends(data):
    """The absolute end of every field of every non-empty row, row by row."""
    out = []
    for start, _, fields in walk(bytes(data))[1]:
        ends, at = [], start
        for f in fields:
            at += len(f)
            ends.append(at)
            at += 1
        out.append(tuple(ends))
    return out


# ---- mutants of one good file (tests/test_matches_restated_host.py asserts their spread) ----

MUTANTS = 400
MUTANT_SEEDS = {"0": 20250, "1": 20251}             # per FS_MATCHES_STAGE setting
MUTANT_BYTES = b'",\r\n\x00\x80\xc3\xe4\xed\xf0\xf4' + b'7-+.e '
MUTANT_OPS = ('replace', 'insert', 'delete', 'duplicate')
MUTANT_OP_WEIGHTS = (0.4, 0.4, 0.1, 0.1)
EDGES = (64, 4096, 16384)


def base_file():
    """odd_rows() and some_rows() of tests/test_gpu_matches.py behind a header row, CRLF, a
    little over two tiles (about 36 KiB)."""
    from tests.test_gpu_matches import csv_bytes, odd_rows, some_rows
    return csv_bytes(odd_rows() + some_rows(410, seed=23), header=True)


def mutant_positions(rng, n, count):
    """Half uniform; half within 4 bytes of a multiple of 64, 4096 or 16384 or of either end."""
    out = rng.integers(0, n, count).tolist()
    for k in range(count // 2, count):
        kind = int(rng.integers(0, 5))
        if kind < 3:
            e = EDGES[kind]
            at = e * int(rng.integers(1, (n - 1) // e + 1))
        else:
            at = 0 if kind == 3 else n
        out[k] = min(max(at + int(rng.integers(-4, 5)), 0), n - 1)
    return out


def mutants(stage):
    """[(what, bytes), ...]: MUTANTS single-byte changes of base_file() for one stage setting."""
    base = base_file()
    rng = np.random.default_rng(MUTANT_SEEDS[stage])
    positions = mutant_positions(rng, len(base), MUTANTS)
    ops = rng.choice(len(MUTANT_OPS), size=MUTANTS, p=MUTANT_OP_WEIGHTS).tolist()
    picks = rng.integers(0, len(MUTANT_BYTES), MUTANTS).tolist()
    digits = rng.integers(0, 10, MUTANTS).tolist()
    out = []
    for at, op, pick, digit in zip(positions, ops, picks, digits):
        b = MUTANT_BYTES[pick:pick + 1]
        if b == b'7':
            b = b'%d' % digit
        op = MUTANT_OPS[op]
        if op == 'replace':
            data = base[:at] + b + base[at + 1:]
        elif op == 'insert':
            data = base[:at] + b + base[at:]
        elif op == 'delete':
            data = base[:at] + base[at + 1:]
        else:
            data = base[:at + 1] + base[at:]
        out.append(("%s %r at %d" % (op, b if op in ('replace', 'insert') else base[at:at + 1], at),
                    data))
    return out
