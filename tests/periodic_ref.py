"""CRC-32 reference for spans of a periodic image, at no cost in the span length.

The GPU tests of records up to 2^32-1 bytes (test_gpu_crc_long.py) cannot
afford a 4 GiB host image or a byte-by-byte oracle pass over one.  Their
device image is one block B of p bytes repeated, image[a] = B[a % p], so the
CRC of image[off : off+length) is

    head (the rest of the period holding `off`)
    || k whole blocks
    || tail (a prefix of B)

with each piece from the standard library's zlib.crc32 and the pieces joined
by the CRC combination law, in zlib's convention (finalised CRCs):

    crc(A || B) = crc(A) (x) x^(8|B|)  xor  crc(B)      in GF(2)[x] mod P

The product is a 32-step reflected multiply mod 0xEDB88320 (bit 31 is x^0),
x^(8n) comes from square-and-multiply starting at x^8 = 0x00800000, and the k
whole blocks by doubling.  Nothing here uses the project's own CRC code
(lsmck_crc32_combine, lsm_storage_engine_amd.crc32): tests/test_periodic_ref.py
checks this module against running zlib.crc32 alone.
"""
import zlib

POLY = 0xEDB88320
X0 = 0x80000000  # x^0
X8 = 0x00800000  # x^8


def gf2_mul(a, b):
    """a(x) * b(x) mod P(x), reflected: bit 31 is the coefficient of x^0."""
    p = 0
    for i in range(32):
        if a & (X0 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x_pow8(n):
    """x^(8n) mod P(x)."""
    r, sq = X0, X8
    while n:
        if n & 1:
            r = gf2_mul(r, sq)
        sq = gf2_mul(sq, sq)
        n >>= 1
    return r


def combine(crc_a, crc_b, len_b):
    """crc(A || B) from crc(A), crc(B) and |B|."""
    return gf2_mul(crc_a, x_pow8(len_b)) ^ crc_b


def _repeat(crc_b, p, k):
    """(crc, length) of k copies of a block of p bytes whose CRC is crc_b."""
    rc, rl = 0, 0          # the empty string
    pc, pl = crc_b, p      # 2^j copies
    while k:
        if k & 1:
            rc, rl = combine(rc, pc, pl), rl + pl
        pc, pl = combine(pc, pc, pl), 2 * pl
        k >>= 1
    return rc, rl


_whole = {}  # id(block) -> (block, crc of the whole block): one zlib pass per block object


def _block_crc(block, mv):
    hit = _whole.get(id(block))
    if hit is None or hit[0] is not block:
        _whole.clear()
        hit = _whole[id(block)] = (block, zlib.crc32(mv))
    return hit[1]


def _clean(block, mv, off, length):
    """CRC of image[off : off+length) with no patch inside."""
    p = len(mv)
    s = off % p
    head = min(length, p - s)
    crc = zlib.crc32(mv[s:s + head])
    left = length - head
    k, tail = divmod(left, p)
    if k:
        rc, rl = _repeat(_block_crc(block, mv), p, k)
        crc = combine(crc, rc, rl)
    if tail:
        crc = combine(crc, zlib.crc32(mv[:tail]), tail)
    return crc


def periodic_crc(block, off, length, patches=()):
    """CRC-32 (zlib / ISO-HDLC) of image[off : off+length), image[a] =
    block[a % len(block)], with the bytes of `patches` -- (absolute offset,
    byte) pairs -- overriding the image.  Patches outside the span are
    ignored; of two patches of one offset the last wins."""
    mv = memoryview(block).cast("B")
    end = off + length
    inside = dict((a, b) for a, b in patches if off <= a < end)
    crc, pos = 0, off
    for a in sorted(inside):
        crc = combine(crc, _clean(block, mv, pos, a - pos), a - pos)
        crc = combine(crc, zlib.crc32(bytes([inside[a] & 0xFF])), 1)
        pos = a + 1
    return combine(crc, _clean(block, mv, pos, end - pos), end - pos)
