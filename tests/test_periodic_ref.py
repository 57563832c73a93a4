"""The periodic-image CRC reference (periodic_ref.py) against running
zlib.crc32 over the same bytes, period by period -- nothing of the project's
own CRC code on either side.  The GPU tests of records up to 2^32-1 bytes
rest on this reference, so it is pinned here on the CPU first: short and
multi-period spans, spans with patched bytes (the WAL corruption cases), and
one anchor at the full 2^32-1 bytes (no 4 GiB allocation: zlib runs over the
one period again and again, a few seconds)."""
import time
import zlib

import pytest

from oracle import oracle as O
from periodic_ref import combine, gf2_mul, periodic_crc, x_pow8

P = (12 << 20) + 64
SEED = 0x5EED0041

SPANS = [(0, 0), (5, 1), (P - 1, 2), (3, 3 * P + 17), (77, (40 << 20) + 5)]


@pytest.fixture(scope="module")
def block():
    return O.gen_stream(SEED, 0, P).tobytes()


def running_crc(block, off, length, patches=()):
    """zlib.crc32 fed the span's bytes piece by piece, each piece at most the
    rest of its period, patched bytes written into a copy of the piece."""
    p = len(block)
    pat = dict(patches)
    c, pos, end = 0, off, off + length
    while pos < end:
        s = pos % p
        m = min(end - pos, p - s)
        hit = [a for a in pat if pos <= a < pos + m]
        if hit:
            piece = bytearray(block[s:s + m])
            for a in hit:
                piece[a - pos] = pat[a]
        else:
            piece = memoryview(block)[s:s + m]
        c = zlib.crc32(piece, c)
        pos += m
    return c


def _patch_sets(off, length):
    """no patch; one patch; two patches -- the first and the last byte among
    them, and patches outside the span (ignored)"""
    first, last = off, off + length - 1
    sets = [[]]
    if length == 0:
        return sets + [[(off, 0x5A)], [(off - 1 if off else 0, 1), (off + 1, 2)]]
    mid = off + length // 2
    sets += [[(first, 0xA5)], [(last, 0x00)], [(mid, 0xFF)]]
    sets += [[(first, 0x01), (last, 0x02)], [(mid, 0x10), (last + 1, 0x20)]]
    if length > P + 9:  # the same block byte patched in one period and not in the next
        sets += [[(off + 7, 0x33), (off + 7 + P, 0x44)], [(off + P - 1, 0x77), (off + P, 0x88)]]
    return sets


@pytest.mark.parametrize("off,length", SPANS)
def test_periodic_crc_matches_running_zlib(block, off, length):
    for patches in _patch_sets(off, length):
        # a patch that writes the byte already there must change nothing: use its complement
        patches = [(a, (block[a % P] ^ 0xFF) if b == 0xFF else b) for a, b in patches]
        want = running_crc(block, off, length, patches)
        assert periodic_crc(block, off, length, patches) == want, (off, length, patches)
        if patches and any(off <= a < off + length and block[a % P] != b for a, b in patches):
            assert want != running_crc(block, off, length), "the patch must change the CRC"


def test_combine_algebra():
    assert x_pow8(0) == 0x80000000 and x_pow8(1) == 0x00800000
    assert gf2_mul(0x80000000, 0x12345678) == 0x12345678
    a, b = b"hello, ", b"world" * 1000
    assert combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
    assert combine(zlib.crc32(a), 0, 0) == zlib.crc32(a)
    assert combine(0, zlib.crc32(b), len(b)) == zlib.crc32(b)


def test_accepts_array_blocks(block):
    import numpy as np
    arr = np.frombuffer(block, dtype=np.uint8)
    assert periodic_crc(arr, P - 3, 10) == zlib.crc32(block[-3:] + block[:7])


def test_anchor_full_length(block):
    """(off 3, len 2^32-1): the length the GPU tests depend on."""
    off, length = 3, (1 << 32) - 1
    t0 = time.perf_counter()
    got = periodic_crc(block, off, length)
    t1 = time.perf_counter()
    want = running_crc(block, off, length)
    t2 = time.perf_counter()
    print(f"anchor: periodic_crc {t1 - t0:.3f} s, running zlib {t2 - t1:.2f} s")
    assert got == want
