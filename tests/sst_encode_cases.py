"""Batches for the batch SSTable encode's tests (test_gpu_sst_encode.py).

lsmck_sstable_encode_batch turns entries -- key and value ranges in two arenas,
cut into tables by table_first -- into the tables' data files, back to back in
one arena, their bincode index files in another, and a SHA-256 per file.  Its
gather kernel (lsmck_sstable.hip sst_gather) cuts the data arena into tiles of
T bytes and chunks of 16, both aligned on the arena's address, and branches on
where a chunk lies in its record (header, key, value, or across a boundary),
on the source's alignment and on the tile's first record.  Each batch below
walks one of these spaces.  The expected bytes come from struct.pack and
hashlib alone (Batch.expected), as tests/golden/make_golden.py:sstable_files
writes them: nothing of the library computes them.

Nothing in this module needs a GPU: tests/test_sst_encode_cases.py checks that
the batches reach the edges they claim, for every tile size the kernel may use.
"""
import hashlib
import struct

import numpy as np

from lsm_storage_engine_amd import _lib
from oracle import oracle as O
from wal_encode_cases import GUARD, TILES, BIG_SEED, BIG_VALUE, commands, crc_concat  # noqa: F401

HDR = 8           # [u32 klen][u32 vlen]
INDEX_STEP = 100  # src/tokio/sstable.rs:17


class Batch:
    def __init__(self, name, keys, vals, ents, first):
        self.name = name
        self.keys = np.ascontiguousarray(keys, dtype=np.uint8)
        self.vals = self.keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        self.ents = np.ascontiguousarray(ents, dtype=_lib.WAL_CMD_DTYPE)
        self.first = np.ascontiguousarray(first, dtype=np.uint64)
        assert self.first[0] == 0 and self.first[-1] == len(self.ents) and (np.diff(self.first.astype(np.int64)) >= 0).all()
        self._expected = None

    def __len__(self):
        return len(self.ents)

    def __repr__(self):
        return f"Batch({self.name}, n={len(self.ents)}, ntab={self.ntab})"

    @property
    def ntab(self):
        return len(self.first) - 1

    def sizes(self):
        c = self.ents
        return np.uint64(HDR) + c["klen"].astype(np.uint64) + c["vlen"].astype(np.uint64)

    def rec_off(self):
        """Every record's offset in the data arena, and the arena's size."""
        s = self.sizes()
        e = np.cumsum(s, dtype=np.uint64)
        return e - s, int(e[-1]) if len(e) else 0

    def key(self, i):
        c = self.ents[i]
        return self.keys[int(c["key_off"]):int(c["key_off"]) + int(c["klen"])].tobytes()

    def val(self, i):
        c = self.ents[i]
        return self.vals[int(c["val_off"]):int(c["val_off"]) + int(c["vlen"])].tobytes()

    def table(self, t):
        return [(self.key(i), self.val(i)) for i in range(int(self.first[t]), int(self.first[t + 1]))]

    def sorted_tables(self):
        """Every table's keys increase strictly (bytes compare as the reference's Vec<u8> keys do)."""
        for t in range(self.ntab):
            ks = [self.key(i) for i in range(int(self.first[t]), int(self.first[t + 1]))]
            if any(a >= b for a, b in zip(ks, ks[1:])):
                return False
        return True

    def sizes_only(self):
        """(data bytes, index bytes) from the lengths alone."""
        c = self.ents
        index = 8 * self.ntab
        for t in range(self.ntab):
            i = np.arange(int(self.first[t]), int(self.first[t + 1]), INDEX_STEP)
            index += 16 * len(i) + int(c["klen"][i].sum())
        return self.rec_off()[1], index

    def expected(self):
        """(data, index, spans, data_sha, index_sha): the tables' files back
        to back, where each lies (SSTABLE_SPAN_DTYPE) and its SHA-256, computed once."""
        if self._expected is None:
            data, index = bytearray(), bytearray()
            spans = np.zeros(self.ntab, dtype=_lib.SSTABLE_SPAN_DTYPE)
            dsha, isha = np.zeros((self.ntab, 32), np.uint8), np.zeros((self.ntab, 32), np.uint8)
            for t in range(self.ntab):
                d, x = table_files(self.table(t))
                spans[t] = (len(data), len(d), len(index), len(x))
                dsha[t] = np.frombuffer(hashlib.sha256(d).digest(), np.uint8)
                isha[t] = np.frombuffer(hashlib.sha256(x).digest(), np.uint8)
                data += d
                index += x
            self._expected = (np.frombuffer(bytes(data), np.uint8), np.frombuffer(bytes(index), np.uint8), spans,
                              dsha, isha)
        return self._expected


def table_files(entries):
    """One table's data and index file (datafile.rs:27-35; the bincode image of
    sstable_index.rs:42-46's BTreeMap): entries in key order."""
    data, idx, pos = bytearray(), [], 0
    for i, (k, v) in enumerate(entries):
        if i % INDEX_STEP == 0:
            idx.append(struct.pack("<Q", len(k)) + k + struct.pack("<Q", pos))
        data += struct.pack("<II", len(k), len(v)) + k + v
        pos += HDR + len(k) + len(v)
    return bytes(data), struct.pack("<Q", len(idx)) + b"".join(idx)


def entries(key_off, klen, val_off, vlen):
    return commands([1] * len(klen), key_off, klen, val_off, vlen)


def firsts(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def counter_keys(n, width=8, start=0):
    """n keys of `width` bytes, big-endian counters: increasing bytewise."""
    a = np.arange(start, start + n, dtype=np.uint64)
    return np.ascontiguousarray(a.astype(">u8").view(np.uint8).reshape(n, 8)[:, 8 - width:]).ravel()


def packed(name, klen, vlen, sizes, seed, width=None):
    """Counter keys of klen[i] bytes (all `width`, at least 4: distinct and
    increasing) back to back in one arena, values in another."""
    n = len(klen)
    klen, vlen = np.asarray(klen, dtype=np.uint64), np.asarray(vlen, dtype=np.uint64)
    width = int(klen[0]) if width is None and n else width
    assert n == 0 or (klen == width).all() and width >= 4
    keys = counter_keys(n, width) if n else np.zeros(0, np.uint8)
    vals = O.gen_stream(seed, 0, int(vlen.sum()))
    return Batch(name, keys, vals, entries(np.cumsum(klen) - klen, klen, np.cumsum(vlen) - vlen, vlen), firsts(sizes))


def greedy_tables(name, keys, vals, ents, seed, maxtab=12):
    """Cut the entries, in order, into tables of up to `maxtab` (random)
    entries, a new one also before a key its table already holds and before
    a second empty key; then sort every table by key.  Every entry keeps its
    source ranges, so the lengths and residues the entries were made with
    all stay in the batch."""
    rng = np.random.default_rng(seed)
    b = Batch(name, keys, vals, ents, [0, len(ents)])
    order, sizes, cur, seen, limit = [], [], [], set(), int(rng.integers(1, maxtab + 1))
    for i in range(len(ents)):
        k = b.key(i)
        if k in seen or len(cur) >= limit:
            order += sorted(cur, key=b.key)
            sizes.append(len(cur))
            cur, seen, limit = [], set(), int(rng.integers(1, maxtab + 1))
        cur.append(i)
        seen.add(k)
    order += sorted(cur, key=b.key)
    sizes.append(len(cur))
    return Batch(name, b.keys, b.vals, b.ents[order], firsts(sizes))


# --- smallest shapes ---------------------------------------------------------
SMALLEST = ((0, 0), (1, 0), (0, 1), (1, 1))


def smallest():
    """One table of one entry: 8, 9, 9 and 10 bytes."""
    out = []
    for kl, vl in SMALLEST:
        out.append(Batch(f"one_{kl}_{vl}", O.gen_stream(1, 0, 4)[:kl], O.gen_stream(2, 0, 4)[:vl],
                         entries([0], [kl], [0], [vl]), [0, 1]))
    return out


def empty_tables(ntab=5):
    return Batch("empty_tables", np.zeros(0, np.uint8), np.zeros(0, np.uint8), entries([], [], [], []), [0] * (ntab + 1))


def empty_table_places():
    """An empty table first, in the middle (two in a row) and last, around tables of 3, 150 and 2 entries."""
    n = 155
    return packed("empty_table_places", [8] * n, [5 + i % 7 for i in range(n)], [0, 3, 0, 0, 150, 2, 0], 3)


def two_in_a_chunk():
    """Two tables of one 8-byte record (empty key, empty value) each: one 16-byte chunk."""
    return Batch("two_in_a_chunk", np.zeros(0, np.uint8), np.zeros(0, np.uint8), entries([0, 0], [0, 0], [0, 0], [0, 0]),
                 [0, 1, 2])


# --- index step edges --------------------------------------------------------
STEP_SIZES = (1, 99, 100, 101, 199, 200, 201)
STEP_COUNTS = (1, 1, 1, 2, 2, 2, 3)


def index_steps(seed=4):
    """Tables of 1, 99, 100, 101, 199, 200 and 201 entries with keys of 0..40
    bytes (an empty key only as a table's first): the index counts are 1, 1,
    1, 2, 2, 2 and 3."""
    rng = np.random.default_rng(seed)
    ks, vs = [], []
    for t, m in enumerate(STEP_SIZES):
        keys = set()
        if t % 2 == 1:
            keys.add(b"")
        while len(keys) < m:
            keys.add(rng.bytes(int(rng.integers(1, 41))))
        ks += sorted(keys)
        vs += [rng.bytes(int(rng.integers(0, 30))) for _ in range(m)]
    klen, vlen = np.array([len(k) for k in ks], np.uint64), np.array([len(v) for v in vs], np.uint64)
    return Batch("index_steps", np.frombuffer(b"".join(ks), np.uint8), np.frombuffer(b"".join(vs), np.uint8),
                 entries(np.cumsum(klen) - klen, klen, np.cumsum(vlen) - vlen, vlen), firsts(STEP_SIZES))


# --- lengths and alignment ----------------------------------------------------
SLOT = 64  # a source of up to 48 bytes at residue 0..15 fits one 64-byte slot


def lengths_alignment(seed=7, extra=6000):
    """Keys and values of 0..48 bytes at every source residue mod 16: the full
    sweep (length x residue) for keys and for values, then `extra` entries
    with random lengths and residues; the varied sizes move the destination
    through every residue too.  Every source has its own 64-byte slot; the
    entries are cut into small sorted tables (greedy_tables)."""
    rng = np.random.default_rng(seed)
    L, R = np.meshgrid(np.arange(49), np.arange(16), indexing="ij")
    klen = np.concatenate([L.ravel(), rng.integers(0, 49, 784 + extra)])
    kres = np.concatenate([R.ravel(), rng.integers(0, 16, 784 + extra)])
    vlen = np.concatenate([rng.integers(0, 49, 784), L.ravel(), rng.integers(0, 49, extra)])
    vres = np.concatenate([rng.integers(0, 16, 784), R.ravel(), rng.integers(0, 16, extra)])
    n = len(klen)
    slot = np.arange(n) * SLOT
    keys = O.gen_stream(seed, 0, n * SLOT)
    vals = O.gen_stream(seed + 1, 0, n * SLOT)
    return greedy_tables("lengths_alignment", keys, vals, entries(slot + kres, klen, slot + vres, vlen), seed)


def residue_pairs(batch, base=0):
    """(source residue, destination residue) mod 16 of every non-empty key and
    of every non-empty value, the data arena at an address = base mod 16."""
    off, _ = batch.rec_off()
    c = batch.ents
    kd = (off + np.uint64(HDR + base)) % np.uint64(16)
    vd = (off + np.uint64(HDR + base) + c["klen"].astype(np.uint64)) % np.uint64(16)
    km, vm = c["klen"] > 0, c["vlen"] > 0
    kp = set(zip((c["key_off"][km] % np.uint64(16)).tolist(), kd[km].tolist()))
    vp = set(zip((c["val_off"][vm] % np.uint64(16)).tolist(), vd[vm].tolist()))
    return kp, vp


# --- tile edges (T: the kernel's tile bytes; the arena's base a multiple of T) ---
EDGE_KLEN, EDGE_VLEN = 4, 3  # 15-byte records: odd, so every byte of a record meets a tile's first byte


def tile_records(T):
    """2T entries of klen 4, vlen 3 in tables of T, 1, 7 and T - 8 entries:
    every header byte, the key/value boundary and the record boundary meet a
    tile edge, and the second table starts on one (at 15 T)."""
    return packed(f"tile_records_{T}", [EDGE_KLEN] * (2 * T), [EDGE_VLEN] * (2 * T), [T, 1, 7, T - 8], 8)


def edge_phases(batch, T):
    """For every tile edge k*T inside the data arena: that byte's position in its record."""
    off, total = batch.rec_off()
    edges = np.arange(1, (total - 1) // T + 1, dtype=np.uint64) * np.uint64(T)
    r = np.searchsorted(off, edges, side="right") - 1
    return set((edges - off[r]).tolist())


def table_starts(batch):
    """Data arena offsets where a table other than the first starts (with at least one entry before and in it)."""
    off, total = batch.rec_off()
    o = np.concatenate([off, [total]]).astype(np.uint64)
    f = batch.first
    return set(int(o[int(f[t])]) for t in range(1, batch.ntab) if 0 < f[t] < f[t + 1])


def tile_sized(T, k, plus, seed=11):
    """A data arena of exactly k*T + plus bytes: records of 16..130 bytes
    (8-byte counter keys), the last one sized to end there; three tables."""
    rng = np.random.default_rng(seed)
    want = k * T + plus
    vlen, cur = [], 0
    while want - cur > 300:
        vlen.append(int(rng.integers(0, 115)))
        cur += 16 + vlen[-1]
    vlen.append(want - cur - 16)
    n = len(vlen)
    return packed(f"tile_sized_{T}_{k}_{plus}", [8] * n, vlen, [n // 3, n // 3, n - 2 * (n // 3)], seed)


# --- realistic and shared sources ----------------------------------------------
def zipf_tables(n=200_000, seed=0x5EED0003, kmax=64):
    """n sorted entries (16-byte decimal keys, as tree.py's tables) with Zipf
    value lengths (gen_zipf_lengths: 64k - j bytes, k ~ Zipf(1.5) on
    1..kmax), cut into tables of about 4 KiB, 16 KiB, 64 KiB, 256 KiB and 1 MiB in turn."""
    ln = O.gen_zipf_lengths(seed, n, kmax=kmax).astype(np.uint64)
    off = np.cumsum(np.uint64(24) + ln)
    cuts, at, lv = [0], 0, 0
    while cuts[-1] < n:
        at += 4096 << (2 * (lv % 5))
        lv += 1
        cuts.append(max(cuts[-1] + 1, min(n, int(np.searchsorted(off, at)))))
    nums = np.arange(n, dtype=np.int64)
    keys = ((nums[:, None] // (10 ** np.arange(15, -1, -1, dtype=np.int64))[None, :]) % 10 + 48).astype(np.uint8).ravel()
    vals = O.gen_stream(12, 0, int(ln.sum()))
    return Batch("zipf_tables", keys, vals, entries(np.arange(n) * 16, [16] * n, np.cumsum(ln) - ln, ln), cuts)


def shared_arena(n=4000, seed=13):
    """keys == vals: one arena, the entries' keys (12 bytes) and values at
    random, overlapping places in it."""
    rng = np.random.default_rng(seed)
    arena = O.gen_stream(seed, 0, 8192)
    vlen = rng.integers(0, 300, n)
    ko, vo = rng.integers(0, 8192 - 12, n), rng.integers(0, 8192 - 300, n)
    return greedy_tables("shared_arena", arena, arena, entries(ko, [12] * n, vo, vlen), seed, maxtab=300)


def one_value(n=3000, seed=14):
    """Every entry points at one value (777 bytes at an odd offset); keys are 8-byte counters; four tables."""
    vals = O.gen_stream(seed + 1, 0, 1024)
    return Batch("one_value", counter_keys(n), vals, entries(np.arange(n) * 8, [8] * n, [5] * n, [777] * n),
                 [0, 1000, 1001, 2500, n])


# --- errors ----------------------------------------------------------------------
def _ok():
    """Two tables: keys "b", "ba", "bb", "c" | "a", "ab" (order across the boundary is free)."""
    keys = np.frombuffer(b"bbabbcaab", np.uint8)
    vals = O.gen_stream(15, 0, 64)
    return keys, vals, entries([0, 1, 3, 5, 6, 7], [1, 2, 2, 1, 1, 2], [0, 10, 20, 30, 40, 50], [10, 0, 12, 13, 1, 14]), \
        [0, 4, 6]


def ok_across_boundary():
    return Batch("ok_across_boundary", *_ok())


def invalid_cases():
    """(name, batch arguments (keys, vals, ents, first), the first offending
    entry's index, invalid by the entry alone).  Every batch holds valid
    entries around the bad one; `alone` tells whether
    lsmck_sstable_encoded_size refuses the batch too (an entry's type or
    lengths: all it can see)."""
    out = []
    for name, idx, alone in (("type2", 2, True), ("type0", 3, True), ("too_long", 2, True), ("key_past", 5, False),
                             ("val_past", 3, False), ("equal_keys", 2, False), ("prefix_after", 1, False),
                             ("decreasing", 3, False), ("first_of_several", 1, True), ("second_table", 5, False)):
        keys, vals, c, first = _ok()
        if name == "type2":
            c["type"][idx] = 2
        elif name == "type0":
            c["type"][idx] = 0
        elif name == "too_long":  # 8 + klen + vlen = 2^32
            c["klen"][idx], c["vlen"][idx] = 0xFFFFFFF0, 8
        elif name == "key_past":  # one byte past keys_bytes
            c["key_off"][idx] = len(keys) - int(c["klen"][idx]) + 1
        elif name == "val_past":  # one byte past vals_bytes
            c["val_off"][idx] = len(vals) - int(c["vlen"][idx]) + 1
        elif name == "equal_keys":  # "ba", "ba"
            c["key_off"][idx] = 1
        elif name == "prefix_after":  # "b" after "ba": the proper prefix behind the longer key
            c[[0, 1]] = c[[1, 0]]
        elif name == "decreasing":  # "a" behind "bb"
            c["key_off"][idx] = 6
        elif name == "first_of_several":  # entry 1 out of order, entry 3 of type 9, entry 4 past the arena
            c[[0, 1]] = c[[1, 0]]
            c["type"][3] = 9
            c["val_off"][4] = 1 << 40
        else:  # "ab", "a" in the second table
            c[[4, 5]] = c[[5, 4]]
        out.append((name, (keys, vals, c, first), idx, alone))
    return out


def bad_table_firsts(n=6):
    """Malformed table_first arrays for a batch of n entries."""
    return {"not_from_0": [1, 4, n], "not_to_n": [0, 4, n - 1], "past_n": [0, 4, n + 1], "decreasing": [0, 4, 3, n]}


# --- offsets across 2^32 ---------------------------------------------------------
def big_entries(nbig=70, nsmall=1000, seed=17):
    """70 entries whose values are all the one 64 MiB arena, then 1000 small
    ones (values of 0..99 bytes from the arena's start), with 8-byte counter
    keys, in five tables: a data arena of about 4.4 GiB from small sources.
    Returns (keys arena, entries, table_first); the value arena is
    O.gen_stream(BIG_SEED, 0, BIG_VALUE)."""
    rng = np.random.default_rng(seed)
    n = nbig + nsmall
    vlen = np.concatenate([np.full(nbig, BIG_VALUE), rng.integers(0, 100, nsmall)])
    voff = np.concatenate([np.zeros(nbig, dtype=np.int64), rng.integers(0, 1000, nsmall)])
    return counter_keys(n), entries(np.arange(n) * 8, [8] * n, voff, vlen), \
        np.array([0, 30, 64, 66, nbig + 350, n], dtype=np.uint64)  # (the third table starts past 4 GiB)
