#!/usr/bin/env python3
"""Writes fs_pow5.h: 128-bit approximations of 5^q for q = -342 .. 308, the table behind the
decimal-to-double conversion of fs_dec.h (D. Lemire, "Number parsing at a gigabyte per second",
Software: Practice and Experience 51 (8), 2021, section 5 and appendix B).

q >= 0: the 128 most significant bits of 5^q (5^q shifted until it lies in [2^127, 2^128),
truncated).  q < 0: 2^b / 5^-q rounded up, b chosen so that the result has 128 bits.  Each entry
is written as two 64-bit words, the high one first.

    python3 gen_pow5.py > fs_pow5.h
"""

Q_MIN, Q_MAX = -342, 308


def entry(q):
    if q >= 0:
        c = 5 ** q
        while c < 1 << 127:
            c *= 2
        while c >= 1 << 128:
            c //= 2
        return c
    power5 = 5 ** -q
    z = 0
    while (1 << z) < power5:
        z += 1
    if q >= -27:
        return 2 ** (z + 127) // power5 + 1
    c = 2 ** (2 * z + 128) // power5 + 1
    while c >= 1 << 128:
        c //= 2
    return c


def main():
    print("// fs_pow5.h -- written by gen_pow5.py, not by hand: 5^q, q = %d .. %d, as 128-bit" % (Q_MIN, Q_MAX))
    print("// approximations {high, low}.  Included by fs_dec.h once per address space (no guard).")
    print("FS_POW5_QUAL const uint64_t fs_pow5_128[2 * %d] = {" % (Q_MAX - Q_MIN + 1))
    for q in range(Q_MIN, Q_MAX + 1):
        c = entry(q)
        assert 1 << 127 <= c < 1 << 128
        print("    0x%016xull, 0x%016xull,  // 5^%d" % (c >> 64, c & ((1 << 64) - 1), q))
    print("};")


if __name__ == "__main__":
    main()
