"""The model for an opened table set's resident bloom filters ("bloom_bits"),
restated in Python from the definitions and not from csrc/lsmck_bloom.h.

For a table with index items (key_j, pos_j), j < m, and data length L the
KEY SET is every item key (of at most 2^32-1 bytes) and the key of every
record that ``tableset_cases.walk(data, start_j, end_j, cap)`` visits for
j = -1 .. m-1: start_-1 = 0, start_j = pos_j, end_j = pos_{j+1} or L behind
the last item (m == 0: the single walk (0, L)).  The table HAS A FILTER iff
every one of those walks ends within ``cap`` records.

Split-block layout.  nkeys = the item keys + the records visited, duplicates
counted; nblocks = max(1, ceil(nkeys * bits / 256)) blocks of eight u32 words
(2^32 blocks or more: no filter).  mix is splitmix64's finaliser;
h = mix(klen * 0x9E3779B97F4A7C15 mod 2^64), then h = mix(h ^ w) for every
8-byte little-endian word w of the key, the last one zero-padded.  The block is
((h >> 32) * nblocks) >> 32 and, with x the low 32 bits of h, word i carries
bit (x * SALT[i] mod 2^32) >> 27.

A (query, table) pair is BLOOMED iff it is not fenced (tableset_cases.Fence),
the table has a filter and the filter does not hold the key.
tests/test_bloom_cases.py proves filter-negative => get_cases.table_get is
None, so the GPU tests may rely on the counts; nothing here imports the
library."""
import get_cases as G
import tableset_cases as T

M64 = (1 << 64) - 1
SALT = (0x47b6137b, 0x44974d91, 0x8824ad5b, 0xa2b7289d, 0x705495c7, 0x2df1424b, 0x9efc4947, 0x5c6bfb31)


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_hash(key):
    h = mix((len(key) * 0x9E3779B97F4A7C15) & M64)
    for i in range(0, len(key), 8):
        h = mix(h ^ int.from_bytes(key[i:i + 8], "little"))
    return h


def block_bits(h, nblocks):
    """(the block, its eight bit numbers) of the hash h."""
    x = h & 0xFFFFFFFF
    return ((h >> 32) * nblocks) >> 32, [((x * s) & 0xFFFFFFFF) >> 27 for s in SALT]


def key_set(data, index, cap=T.CAP):
    """(every walk ended within cap, the keys with duplicates): the item keys, then every walk's records."""
    keys, pos = G.btreemap(index)
    out = [k for k in keys if len(k) < 1 << 32]
    starts, ends = [0] + list(pos), list(pos) + [len(data)]
    ok = True
    for s, e in zip(starts, ends):
        ended, seen = T.walk(data, s, e, cap)
        ok = ok and ended
        out += seen
    return ok, out


def nblocks(nkeys, bits):
    return max(1, -(-nkeys * bits // 256))


class Filter:
    """One table's filter at ``bits`` per key: ``valid``, ``nkeys``, ``nblocks`` and the blocks' words."""

    def __init__(self, data, index, bits, cap=T.CAP):
        ok, keys = key_set(data, index, cap)
        self.nkeys, self.nblocks = len(keys), nblocks(len(keys), bits)
        self.valid = ok and self.nblocks < 1 << 32
        self.words = {}
        if self.valid:
            for k in keys:
                b, bit = block_bits(key_hash(k), self.nblocks)
                for i in range(8):
                    self.words[8 * b + i] = self.words.get(8 * b + i, 0) | 1 << bit[i]

    def holds(self, key):
        """The filter does not reject the key (always, for a table without one)."""
        if not self.valid:
            return True
        b, bit = block_bits(key_hash(key), self.nblocks)
        return all(self.words.get(8 * b + i, 0) >> bit[i] & 1 for i in range(8))


def has_filter(data, index, cap=T.CAP):
    return key_set(data, index, cap)[0]


def set_stats(tables, bits, cap=T.CAP):
    """{"bloom_tables", "bloom_keys", "blocks"} of the set of (data, index) tables."""
    f = [Filter(d, x, bits, cap) for d, x in tables]
    return {"bloom_tables": sum(x.valid for x in f), "bloom_keys": sum(x.nkeys for x in f if x.valid),
            "blocks": sum(x.nblocks for x in f if x.valid)}


def count_bloomed(tables, keys, bits, cap=T.CAP):
    """The (query, table) pairs that pass the fences and that the filters drop."""
    fences = [T.Fence(d, x, cap) for d, x in tables]
    filters = [Filter(d, x, bits, cap) for d, x in tables]
    return sum(1 for k in keys for fe, fi in zip(fences, filters) if not fe.fenced(k) and not fi.holds(k))


# --- shapes the GPU tests share -----------------------------------------------------------
def key16(x):
    """x as a 16-byte key: eight zero bytes, then x big-endian -- every compare ties past 8 bytes."""
    return bytes(8) + x.to_bytes(8, "big")


def interleaved(m=1000, ntab=4, nq=4000, seed=15):
    """4 tables of 1,000 entries whose keys interleave -- table t holds 8 i + t
    -- and 4,000 queries, half of them absent (8 i + 4 .. 8 i + 7), all with
    0 < i < m - 1 and so between every table's first and last key: no pair is
    fenced.  (tables' entries, query keys)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    tables = [[(key16(8 * i + t), b"v%d-%d" % (t, i)) for i in range(m)] for t in range(ntab)]
    i, t = rng.integers(1, m - 1, nq), rng.integers(0, ntab, nq)
    return tables, [key16(8 * int(a) + int(b) + (4 if j % 2 else 0)) for j, (a, b) in enumerate(zip(i, t))]


def key_lengths():
    """One table holding a key of every length 0..24, and queries: those keys
    and of each the last byte changed, one byte longer, one byte shorter."""
    keys = sorted(bytes((7 * n + 3 * j + 1) % 251 for j in range(n)) for n in range(25))
    q, seen = [], set()
    for k in keys:
        for x in [k, k + b"\x00", k + b"\x80"] + ([k[:-1] + bytes([k[-1] ^ 1]), k[:-1] + bytes([k[-1] ^ 0x80]), k[:-1]] if k else []):
            if x not in seen:
                seen.add(x)
                q.append(x)
    return [(k, b"len-%d" % len(k)) for k in keys], q


# the hash of bytes(range(1, n + 1)) for n = 0..24 (the same numbers: tests/native/test_bloom.cpp)
def known_key(n):
    return bytes(range(1, n + 1))
