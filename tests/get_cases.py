"""Cases and expected values for the batch point read
(lsmck_sstable_get_batch, lsmck_sstable_get).

The expected values come from a literal restatement of the reference that
imports nothing from the library:
  * ``btreemap``: the BTreeMap<Vec<u8>, u64> a bincode fixint image holds
    (sstable_index.rs:20-25), with the call's one refusal -- an image that does
    not parse to exactly its length, or whose keys do not strictly increase;
  * ``position_range`` (sstable_index.rs:34-40), ``scan_range``
    (datafile.rs:85-103) and ``table_get`` (sync/sstable.rs:97-113, the bloom
    filter left out: built from the table's own keys it has no false
    negatives); ``read_record`` is merge_cases' (datafile.rs:60-83);
  * ``search``: Db::get_internal's loop over the tables (tokio/db.rs:178-185).
tests/test_get_cases.py proves on the CPU what the GPU tests then rely on: on
tables that sstable.table_bytes writes the restatement equals a dict lookup
(``GetBatch.expected(fast=True)`` uses that for the large seeded batch), and
the quirk cases give the answers worked by hand there.
"""
import bisect
import struct

import numpy as np

from merge_cases import GUARD, SPAN_DTYPE, TOMBSTONE, B, POOL, _File, data_image, fixed_table, index_image, read_record, table

QUERY_DTYPE = np.dtype([("key_off", "<u8"), ("klen", "<u4"), ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([("val_off", "<u8"), ("vlen", "<u4"), ("table", "<u4")])
NONE_TABLE = 0xFFFFFFFF
TOMBSTONE_BIT = 1 << 63
U64_NONE = 2 ** 64 - 1


class RefusedIndex(Exception):
    """The index image is not taken as the map."""


# --- the restatement ------------------------------------------------------------------
def btreemap(index):
    """The map as (sorted keys, positions in key order)."""
    index = bytes(index)
    if len(index) < 8:
        raise RefusedIndex("no count")
    count, at, keys, pos = struct.unpack_from("<Q", index, 0)[0], 8, [], []
    for _ in range(count):
        if len(index) - at < 8:
            raise RefusedIndex("an item's length is cut")
        klen = struct.unpack_from("<Q", index, at)[0]
        if len(index) - at - 8 < klen or len(index) - at - 8 - klen < 8:
            raise RefusedIndex("an item is cut")
        key = index[at + 8:at + 8 + klen]
        if keys and not keys[-1] < key:
            raise RefusedIndex("keys do not strictly increase")
        keys.append(key)
        pos.append(struct.unpack_from("<Q", index, at + 8 + klen)[0])
        at += 16 + klen
    if at != len(index):
        raise RefusedIndex("trailing bytes")
    return keys, pos


def position_range(m, key, size_bytes):
    """sstable_index.rs:34-40: map.range(..key).next_back() and map.range(key..).next()."""
    keys, pos = m
    i = bisect.bisect_left(keys, key)  # the first item >= key
    start = pos[i - 1] if i > 0 else 0
    end = pos[i] if i < len(keys) else size_bytes
    return start, end


def scan_range(f, key, start, end):
    """datafile.rs:85-103; returns (value offset, value) or None."""
    pos = start
    while True:
        r = read_record(f, pos)
        if r is None:
            return None
        (k, v), length = r
        if k == key:
            return pos + 8 + len(k), v
        pos += length
        if pos >= end:
            return None


def table_get(data, index, key, m=None):
    """SsTable::get: None, or (the value's offset in the data file, the value)."""
    m = btreemap(index) if m is None else m
    f = _File(data)
    keys, pos = m
    i = bisect.bisect_left(keys, key)
    if i < len(keys) and keys[i] == key:  # self.index.get(key): the record there, whatever its key
        r = read_record(f, pos[i])
        return None if r is None else (pos[i] + 8 + len(r[0][0]), r[0][1])
    start, end = position_range(m, key, len(data))
    return scan_range(f, key, start, end)


def search(tables, key, maps=None):
    """get_internal's loop over (data, index) in search order: None, or (table, value offset, value)."""
    for t, (data, index) in enumerate(tables):
        r = table_get(data, index, key, None if maps is None else maps[t])
        if r is not None:
            return (t,) + r
    return None


# --- a batch ------------------------------------------------------------------------
class GetBatch:
    """Tables' images back to back in two arenas of exactly their size (the
    data arena behind ``front`` filler bytes, the last table flush with the
    allocation's end), and the query keys back to back behind ``qfront``
    filler bytes, the last one flush with the end of qkeys."""

    def __init__(self, tables, keys, front=0, qfront=0):
        self.tables, self.keys = [(bytes(d), bytes(x)) for d, x in tables], [bytes(k) for k in keys]
        self.spans = np.zeros(len(tables), dtype=SPAN_DTYPE)
        self.spans["data_len"] = [len(d) for d, _ in self.tables]
        self.spans["index_len"] = [len(x) for _, x in self.tables]
        self.spans["data_off"] = front + np.cumsum(self.spans["data_len"]) - self.spans["data_len"]
        self.spans["index_off"] = np.cumsum(self.spans["index_len"]) - self.spans["index_len"]
        self.data = np.frombuffer(b"\xEE" * front + b"".join(d for d, _ in self.tables), dtype=np.uint8)
        self.index = np.frombuffer(b"".join(x for _, x in self.tables), dtype=np.uint8)
        self.qkeys = np.frombuffer(b"\xDD" * qfront + b"".join(self.keys), dtype=np.uint8)
        self.q = np.zeros(len(self.keys), dtype=QUERY_DTYPE)
        klen = np.array([len(k) for k in self.keys], dtype=np.uint64)
        self.q["klen"] = klen
        self.q["key_off"] = qfront + np.cumsum(klen) - klen

    _memo = {}  # (data, index, key) -> table_get's result: batches that share tables share the work

    def _search(self, key, maps):
        for t, (data, index) in enumerate(self.tables):
            at = (data, index, key)
            if at not in GetBatch._memo:
                GetBatch._memo[at] = table_get(data, index, key, maps[t])
            if GetBatch._memo[at] is not None:
                return (t,) + GetBatch._memo[at]
        return None

    def expected(self, fast=False, entries=None):
        """The results.  fast: from a dict per table (``entries``: the tables'
        sorted pairs) -- for tables table_bytes wrote, where
        tests/test_get_cases.py proves the two equal."""
        res = np.zeros(len(self.keys), dtype=RESULT_DTYPE)
        res["table"] = NONE_TABLE
        if fast:
            dicts = []
            for ents in entries:
                d, pos = {}, 0
                for k, v in ents:
                    d[k] = (pos + 8 + len(k), v)
                    pos += 8 + len(k) + len(v)
                dicts.append(d)
            find = lambda key: next(((t,) + d[key] for t, d in enumerate(dicts) if key in d), None)  # noqa: E731
        else:
            maps = [btreemap(x) for _, x in self.tables]
            find = lambda key: self._search(key, maps)  # noqa: E731  (search(), remembered per table)
        memo = {}
        for i, key in enumerate(self.keys):
            if key not in memo:
                memo[key] = find(key)
            r = memo[key]
            if r is not None:
                t, off, v = r
                off += int(self.spans["data_off"][t])
                res[i] = (off | TOMBSTONE_BIT if v == TOMBSTONE else off, len(v), t)
        return res

    def values(self, res):
        """Per query None or the value's bytes (a tombstone: the byte 0) from a result array."""
        a, out = self.data.tobytes(), []
        for r in res:
            if int(r["table"]) == NONE_TABLE:
                out.append(None)
            else:
                off = int(r["val_off"]) & (TOMBSTONE_BIT - 1)
                out.append(a[off:off + int(r["vlen"])])
        return out


# --- queries ------------------------------------------------------------------------
def below(k):
    """A key just below the non-empty key k."""
    return k[:-1] if k[-1] == 0 else k[:-1] + bytes([k[-1] - 1]) + b"\xff\xff\xff"


def queries_for(entries, light=False):
    """Every present key; absent keys below the first, on both sides of every
    key (so between every adjacent pair and on both sides of every index
    item), above the last, proper prefixes, a present key plus one byte, and
    the empty key (present in some tables, absent in others).  light: the key
    plus one byte for every key (still between every adjacent pair), the
    other neighbours only around the index items."""
    have = set(k for k, _ in entries)
    out = [k for k, _ in entries]
    cand = [b"", b"\xff" * 19]
    for i, (k, _) in enumerate(entries):
        cand.append(k + b"\x00")  # the key plus one byte: its successor in Vec<u8> order
        if k and (not light or i % 100 in (0, 1, 99) or i == len(entries) - 1):
            cand += [below(k), k[:-1], k[:len(k) // 2]]
    seen = set()
    for c in cand:
        if c not in have and c not in seen:
            seen.add(c)
            out.append(c)
    return out


# --- cases ----------------------------------------------------------------------------
SIZES = [0, 1, 99, 100, 101, 199, 200, 201]


def images(entries, step=100):
    return data_image(entries), index_image(entries, step)


def sized_tables():
    """[(name, entries)]: the sizes around the index step with mixed key
    lengths (the serial parse) and with keys of one length (the parallel
    one); seed 0, 2, ... puts the empty key first."""
    out = []
    for j, m in enumerate(SIZES):
        out.append(("mixed %d" % m, table(m, j)))
        out.append(("fixed %d" % m, fixed_table(m, j)))
    return out


def tie_tables():
    """[(name, entries, index step)]: key lengths 0..17 and beyond, keys equal
    in their first 8 bytes that differ later, under an index dense enough
    that the lower bound meets the ties."""
    lens = [B[:n] for n in range(18)]
    ties = [B[:8] + bytes([x]) * n for x in (0, 1, 0x80, 0xff) for n in (1, 2, 5, 9)] + \
        [B[:8] + b"same-tail" + bytes([x]) for x in range(0, 256, 15)] + [B[:12] + b"\x00", B[:12] + b"\x00\x00"]
    pool = sorted(set(POOL + lens + ties))
    ents = [(k, b"v%d" % i if i % 7 else b"") for i, k in enumerate(pool)]
    fixed = sorted(set(B[:8] + bytes([a, b]) for a in (0, 1, 0x7f, 0x80, 0xff) for b in range(0, 256, 17)))
    fents = [(k, b"f%d" % i) for i, k in enumerate(fixed)]
    # 12 + 11 + 13 key bytes: the image has the size of 3 items of 12, so the parallel parse is tried and declines
    pseudo = [(b"a" * 12, b"1"), (b"b" * 11, b"2"), (b"c" * 13, b"3")]
    return [("pseudo uniform", pseudo, 1), ("pool step 1", ents, 1), ("pool step 2", ents, 2), ("pool step 7", ents, 7), ("pool step 100", ents, 100),
            ("ten bytes step 1", fents, 1), ("ten bytes step 3", fents, 3)]


def _items_image(items):
    return struct.pack("<Q", len(items)) + b"".join(struct.pack("<Q", len(k)) + k + struct.pack("<Q", p)
                                                   for k, p in items)


def _positions(entries):
    pos, out = 0, []
    for k, v in entries:
        out.append(pos)
        pos += 8 + len(k) + len(v)
    return out, pos


QUIRK_ENTRIES = [(b"q%05d" % i + b"x" * (i % 4), b"val-%d" % i) for i in range(250)]


def quirk_tables():
    """{name: (data, index)} over QUIRK_ENTRIES (250 entries: items at 0, 100, 200)."""
    e = QUIRK_ENTRIES
    pos, total = _positions(e)
    data = data_image(e)
    k = lambda i: e[i][0]  # noqa: E731
    return {
        "plain": (data, index_image(e)),
        # the item of key 100 points at record 5: the exact hit returns record 5's value
        "other record": (data, _items_image([(k(0), 0), (k(100), pos[5]), (k(200), pos[200])])),
        # positions at and past data_len, and 4 bytes before the end (no header fits)
        "pos at end": (data, _items_image([(k(0), 0), (k(100), total), (k(200), pos[200])])),
        "pos past end": (data, _items_image([(k(0), 0), (k(100), 2 ** 63 + 5), (k(200), pos[200])])),
        "pos max": (data, _items_image([(k(0), 0), (k(100), U64_NONE), (k(200), pos[200])])),
        "pos cut header": (data, _items_image([(k(0), 0), (k(100), total - 4), (k(200), pos[200])])),
        # in the middle of record 100's key: the 8 bytes there read as lengths no file holds
        "pos mid record": (data, _items_image([(k(0), 0), (k(100), pos[100] + 9), (k(200), pos[200])])),
        # the item of key 100 removed: an interval of 200 records
        "item removed": (data, _items_image([(k(0), 0), (k(200), pos[200])])),
        # positions that do not increase: for keys between items 1 and 2 start = pos[150] >= end = pos[100]
        "start past end": (data, _items_image([(k(0), 0), (k(100), pos[150]), (k(200), pos[100])])),
    }


def cut_tables():
    """[(cut, (data, index), entries)]: a table of 5 entries whose data file is cut at every byte of its last record."""
    e = [(b"c%d" % i + b"y" * i, b"w" * (3 * i + 1)) for i in range(5)]
    data, index = images(e)
    pos, total = _positions(e)
    return [(cut, (data[:cut], index), e) for cut in range(pos[4], total + 1)]


def refused_indexes():
    """[(name, index image)] over QUIRK_ENTRIES: every index the call refuses."""
    e = QUIRK_ENTRIES
    pos, _ = _positions(e)
    x = index_image(e)
    k = lambda i: e[i][0]  # noqa: E731
    return [("short", x[:-1]), ("long", x + b"\x00"), ("count+1", struct.pack("<Q", 4) + x[8:]),
            ("count huge", struct.pack("<Q", 2 ** 61) + x[8:]), ("count-1", struct.pack("<Q", 2) + x[8:]),
            ("no count", x[:7]), ("empty", b""),
            ("equal keys", _items_image([(k(0), 0), (k(100), pos[100]), (k(100), pos[200])])),
            ("out of order", _items_image([(k(0), 0), (k(200), pos[200]), (k(100), pos[100])])),
            ("prefix after", _items_image([(k(100) + b"a", 0), (k(100), pos[100])])),
            ("klen past the end", struct.pack("<QQ", 1, 2 ** 40) + b"abc" + struct.pack("<Q", 0))]


def refused_fixed_indexes():
    """The same for an index of one key length (the parallel parse)."""
    e = fixed_table(450, 3)
    pos, _ = _positions(e)
    x = index_image(e)
    items = [(e[i][0], pos[i]) for i in range(0, 450, 100)]
    swapped = items[:2] + [items[3], items[2]] + items[4:]
    return e, [("short", x[:-1]), ("long", x + b"\x00"), ("count+1", struct.pack("<Q", 6) + x[8:]),
               ("equal keys", _items_image(items[:3] + [items[2]] + items[4:])),
               ("out of order", _items_image(swapped)),
               # item 1's length field is 13: the image still has the size of 5 items of one length, the items are
               # not where that puts them, and the serial parse then runs off the end
               ("one klen off", x[:8 + 28] + struct.pack("<Q", 13) + x[8 + 28 + 8:])]


def several_tables():
    """(tables' entries in search order, queries): a key in tables 0 and 2, a
    tombstone in table 0 over a live value in table 1, a key in the last
    table only, a key in none, duplicate queries."""
    t0 = [(b"both", b"zero"), (b"dead", TOMBSTONE), (b"only0", b"0")]
    t1 = [(b"dead", b"alive-in-1"), (b"mid", b"\x00\x00")]
    t2 = [(b"both", b"two"), (b"empty", b"")]
    t3 = [(b"last", b"three"), (b"tomb3", TOMBSTONE)]
    keys = [b"both", b"dead", b"last", b"none", b"both", b"both", b"mid", b"empty", b"tomb3", b"only0", b"", b"dead",
            b"none"]
    return [t0, t1, t2, t3], keys


def seeded_batch(seed=11, ntab=64, nq=4096):
    """64 tables of 1..1000 entries over overlapping key ranges and 4096
    queries, about half present: (tables' entries, query keys)."""
    rng = np.random.default_rng(seed)
    tables, present = [], []
    for t in range(ntab):
        m = int(rng.integers(1, 1001)) if t not in (0, 1) else (1, 1000)[t]
        nums = np.sort(rng.choice(40000, size=m, replace=False))
        ents = []
        for j, x in enumerate(nums.tolist()):
            k = b"key%08d" % x + b"s" * (x % 5)
            v = TOMBSTONE if (x + t) % 13 == 0 else b"t%d-" % t + b"v" * (x % 23)
            ents.append((k, v))
        ents.sort()
        tables.append(ents)
        present += [k for k, _ in ents]
    keys = []
    for i in range(nq):
        if i % 2:
            keys.append(present[int(rng.integers(0, len(present)))])
        else:
            x = int(rng.integers(0, 40000))
            keys.append(b"key%08d" % x + b"s" * ((x + 1) % 5) + (b"" if i % 4 else b"!"))
    return tables, keys
