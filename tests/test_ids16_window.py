"""The ids of one window out of a 16-bit id array, as k_scan_rows' verification takes them from a
batch's 16-bit copy (fs_ids16.h, fs_ids16_window: aligned 32-bit words from the even position
p & ~1, shifted down by one id when p is odd), through the host entry fs_debug_ids16_window and
held against plain numpy slicing: every n = 2..8 at both parities of p.  The arrays alternate 0
and 65 535 in both orders, so a swapped half-word or a shift by one id shows in every slot; a
second pair holds distinct ids.  No GPU is involved."""
import ctypes as C

import numpy as np
import pytest

from fandom_search_amd import _lib, abi

PAD = 16                      # zeroed ids behind the array (the device copy has fs_scan_pad_tokens() of them)
SIZES = (2, 3, 4, 5, 6, 7, 8)


def _window(L, buf, p, n):
    out = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    rc = L.fs_debug_ids16_window(buf.ctypes.data_as(C.POINTER(C.c_uint16)), p, n,
                                 out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == abi.FS_OK
    assert (out[n:] == 0xDEADBEEF).all(), "wrote behind the window's n ids"
    return out[:n]


def _arrays(length):
    """`length` ids in front of a zeroed pad: 0 / 65 535 alternating in both orders, pairs of
    each, and distinct ids (position and a high bit)."""
    i = np.arange(length)
    forms = [np.where(i % 2 == 0, 0, 65535), np.where(i % 2 == 0, 65535, 0),
             np.where(i // 2 % 2 == 0, 0, 65535), np.where(i // 2 % 2 == 0, 65535, 0),
             (i * 257 + 1) % 65536, 65535 - i % 65536]
    out = []
    for f in forms:
        buf = np.zeros(length + PAD, dtype=np.uint16)
        buf[:length] = f.astype(np.uint16)
        out.append(buf)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_every_position_of_an_odd_and_an_even_array(n):
    """Every p with a whole window inside the array -- p = 0 and 1, both parities, and the last
    window of an array of odd and of even length, whose aligned read runs into the zeroed pad."""
    L = _lib.load()
    for length in (40, 41):
        for buf in _arrays(length):
            assert buf.ctypes.data % 4 == 0
            for p in range(0, length - n + 1):
                got = _window(L, buf, p, n)
                assert got.tolist() == buf[p:p + n].astype(np.uint32).tolist(), (length, p, n)


@pytest.mark.parametrize("n", SIZES)
def test_the_ids_come_zero_extended(n):
    """65 535 in every slot: nothing of a neighbour is left in an id's upper half."""
    L = _lib.load()
    buf = np.zeros(32 + PAD, dtype=np.uint16)
    buf[:32] = 65535
    for p in (0, 1, 32 - n - 1, 32 - n):
        assert _window(L, buf, p, n).tolist() == [65535] * n
    # the window that ends at the array's end takes nothing from the pad, the one behind it does
    assert _window(L, buf, 32 - n + 1, n).tolist() == [65535] * (n - 1) + [0]


def test_window_sizes_outside_2_to_8_are_refused():
    L = _lib.load()
    buf = np.zeros(32, dtype=np.uint16)
    out = np.zeros(8, dtype=np.uint32)
    for n in (0, 1, 9):
        assert L.fs_debug_ids16_window(buf.ctypes.data_as(C.POINTER(C.c_uint16)), 0, n,
                                       out.ctypes.data_as(C.POINTER(C.c_uint32))) == abi.FS_E_INVALID
    assert L.fs_debug_ids16_window(None, 0, 6, out.ctypes.data_as(C.POINTER(C.c_uint32))) == abi.FS_E_INVALID
