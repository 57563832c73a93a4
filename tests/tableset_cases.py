"""Cases and the model for the opened table set (lsmck_tableset_open,
lsmck_tableset_get_batch): the key fences restated over get_cases.

For a table with index items (key_j, pos_j), j < m, and data length L:
  * low (m >= 1): walk what scan_range(0, pos_0) visits when nothing matches
    -- the record at 0 is attempted even when pos_0 is 0, then the walk goes
    on while pos < pos_0 and a whole record fits.  Valid iff the walk ends
    within ``cap`` records and no visited key is below key_0; then every
    k < key_0 is None.
  * high (m >= 1): the walk of scan_range(pos_{m-1}, L) by the same rule.
    Valid iff it ends within the cap; hi = max(key_{m-1}, the visited keys);
    then every k > hi is None.
  * m == 0: no fence.
A (query, table) pair is FENCED iff (low valid and k < key_0) or (high valid
and k > hi).  tests/test_tableset_cases.py proves fenced => get_cases.table_get
is None for every case table and key, so the GPU tests may rely on the model's
counts; nothing here imports the library.
"""
import struct

import numpy as np

import get_cases as G
from merge_cases import TOMBSTONE, _File, data_image, index_image, read_record

CAP = 256  # "fence_walk_cap"'s default


def walk(data, start, end, cap):
    """(ended within cap, the visited keys): what scan_range(start, end) visits when nothing matches."""
    f, pos, seen = _File(data), start, []
    while True:
        r = read_record(f, pos)
        if r is None:
            return True, seen
        if len(seen) == cap:
            return False, seen
        (k, _), length = r
        seen.append(k)
        pos += length
        if pos >= end:
            return True, seen


class Fence:
    """One table's fences: ``low`` (key_0 or None) and ``high`` (hi or None)."""

    def __init__(self, data, index, cap=CAP):
        keys, pos = G.btreemap(index)
        self.low = self.high = None
        if not keys:
            return
        ok, seen = walk(data, 0, pos[0], cap)
        if ok and all(k >= keys[0] for k in seen):
            self.low = keys[0]
        ok, seen = walk(data, pos[-1], len(data), cap)
        if ok:
            self.high = max([keys[-1]] + seen)

    def fenced(self, key):
        return (self.low is not None and key < self.low) or (self.high is not None and key > self.high)


def count_fenced(tables, keys, cap=CAP):
    """The (query, table) pairs the fences drop."""
    fences = [Fence(d, x, cap) for d, x in tables]
    return sum(1 for k in keys for f in fences if f.fenced(k))


def around(k):
    """Queries equal to, just below and just above the key k."""
    out = [k, k + b"\x00"]
    if k:
        out += [G.below(k), k[:-1]]
    return out


# --- doctored tables --------------------------------------------------------------------
def _items(items):
    return struct.pack("<Q", len(items)) + b"".join(struct.pack("<Q", len(k)) + k + struct.pack("<Q", p)
                                                   for k, p in items)


def _pos(entries):
    return G._positions(entries)


def doctored(cap=CAP):
    """{name: ((data, index), queries)}: tables no writer makes, each with
    queries equal to, just below and just above key_0, hi and the last
    record's key, the empty key and a key above everything."""
    out = {}

    def add(name, data, items, extra=()):
        index = _items(items)
        f = Fence(data, index, cap)
        keys = [b"", b"\xff" * 20] + list(extra)
        for k in [items[0][0] if items else None, f.high, _last_key(data)]:
            if k is not None:
                keys += around(k)
        seen, q = set(), []
        for k in keys:
            if k not in seen:
                seen.add(k)
                q.append(k)
        out[name] = ((data, index), q)

    e = [(b"d%04d" % i, b"val%d" % i) for i in range(250)]
    pos, total = _pos(e)
    data = data_image(e)
    k = lambda i: e[i][0]  # noqa: E731
    # the index's first item is missing: pos_0 > 0 and the head keys lie below key_0 -- no low fence, the head answers
    add("first item missing", data, [(k(100), pos[100]), (k(200), pos[200])], [k(0), k(50), k(99), k(100), k(249)])
    # a record at 0 whose key is below key_0 while pos_0 = 0: the query for that key is Some
    low0 = [(b"a-low", b"found-below-key0")] + e[1:]
    add("low record at 0", data_image(low0), [(k(0), 0)] + [(k(i), _pos(low0)[0][i]) for i in (100, 200)],
        [b"a-low", k(0), k(1)])
    # an unsorted tail whose maximum is not its last record
    tail = e[:200] + [(b"d0200", b"x"), (b"zz-max", b"top"), (b"d0100a", b"back"), (b"m-last", b"end")]
    tpos, _ = _pos(tail)
    add("unsorted tail", data_image(tail), [(k(0), 0), (k(100), tpos[100]), (k(200), tpos[200])],
        [b"zz-max", b"zz-max\x00", b"m-last", b"d0100a", b"zz"])
    # a tail ending in a cut record (its header and key are there, its value is not)
    add("cut tail", data[:total - 2], [(k(0), 0), (k(100), pos[100]), (k(200), pos[200])], [k(249), k(248)])
    add("cut tail header", data[:pos[249] + 5], [(k(0), 0), (k(100), pos[100]), (k(200), pos[200])], [k(249), k(248)])
    # pos_{m-1} at and past L: no record fits there, hi is key_{m-1} alone
    add("last pos at end", data, [(k(0), 0), (k(100), pos[100]), (k(200), total)], [k(200), k(201), k(249)])
    add("last pos past end", data, [(k(0), 0), (k(100), pos[100]), (k(200), 2 ** 63 + 9)], [k(200), k(201), k(249)])
    add("last pos max", data, [(k(0), 0), (k(200), 2 ** 64 - 1)], [k(200), k(201)])
    # the item at m-1 points at a record whose key is above every item, and the walk from there passes lower keys
    add("last pos at record 5", data, [(k(0), 0), (k(100), pos[100]), (k(200), pos[5])], [k(5), k(6), k(249), k(200)])
    # a head and a tail longer than small caps: 7 records before pos_0, 9 from pos_{m-1}
    long = [(b"h%02d" % i, b"v") for i in range(20)]
    lpos, _ = _pos(long)
    add("long head and tail", data_image(long), [(b"h00", lpos[7]), (b"h11", lpos[11])], [b"h00", b"h06", b"h07", b"h19"])
    # exactly 4 records in the head (all >= key_0) and 4 in the tail: a cap of 4 holds, 1 does not
    four = [(b"f%02d" % i, b"w") for i in range(8)]
    fpos, _ = _pos(four)
    add("four and four", data_image(four), [(b"f00", fpos[4]), (b"f04", fpos[4])], [b"f00", b"f03", b"f07", b"e", b"g"])
    # m == 0: no fence, every query walks from 0
    add("no items", data_image(e[:5]), [], [k(0), k(4), k(5)])
    add("no items no data", b"", [])
    # keys that tie past 8 bytes: key_0, hi and the last record share their first 8 bytes (and 16) with the queries
    t = [(b"TIEDKEY-" + s, b"v-" + s) for s in (b"aaaa", b"aaab", b"aaab\x00", b"bbbbbbbbbbbbbbbb", b"bbbbbbbbbbbbbbbc")]
    tp, _ = _pos(t)
    add("ties past 8", data_image(t), [(t[0][0], 0), (t[3][0], tp[3])],
        [b"TIEDKEY-", b"TIEDKEY-aaa", b"TIEDKEY-aaa\xff", b"TIEDKEY-bbbbbbbbbbbbbbbd", b"TIEDKEY-bbbbbbbbbbbbbbbc\x00",
         b"TIEDKEY-bbbbbbbb", b"TIEDKEY", b"TIEDKEY.", b"TIEDKEX\xff"])
    # a key that is a proper prefix of a fence key (covered by around(): k[:-1]) at 7, 8 and 9 bytes
    p = [(b"prefix-89", b"1"), (b"prefix-89abc", b"2")]
    pp, _ = _pos(p)
    add("prefixes", data_image(p), [(p[0][0], 0)], [b"prefix-", b"prefix-8", b"prefix-89a", b"prefix-89abc\x00", b"prefix-89ab"])
    # the empty key as key_0 and as a record behind the last item
    z = [(b"", b"empty-key"), (b"a", TOMBSTONE), (b"b", b"")]
    add("empty key first", data_image(z), [(b"", 0)], [b"", b"\x00", b"a", b"b", b"c"])
    zt = [(b"k1", b"1"), (b"", b"late-empty")]
    add("empty key in the tail", data_image(zt), [(b"k1", 0)], [b"", b"k1", b"k0", b"k2"])
    return out


def _last_key(data):
    f, pos, last = _File(data), 0, None
    while True:
        r = read_record(f, pos)
        if r is None:
            return last
        last = r[0][0]
        pos += r[1]


def doctored_batch(cap=CAP):
    """All doctored tables as ONE search order, asked every table's queries."""
    d = doctored(cap)
    keys, seen = [], set()
    for _, q in d.values():
        for k in q:
            if k not in seen:
                seen.add(k)
                keys.append(k)
    return [t for t, _ in d.values()], keys


# --- the wide order ---------------------------------------------------------------------
WIDE_TABLES, WIDE_RECORDS, WIDE_QUERIES = 300, 40, 2000


def wide_order(seed=14):
    """300 tables of 40 records over disjoint key ranges -- table t holds the
    keys w<t>-<2i> -- and 2,000 queries uniform over the universe (odd numbers
    are absent): (tables' entries, query keys).  One range of 300 holds a key,
    so all but about 1/300 of the pairs are fenced."""
    rng = np.random.default_rng(seed)
    tables = [[(b"w%04d-%04d" % (t, 2 * i), b"t%d-%d" % (t, i) if (t + i) % 9 else TOMBSTONE) for i in range(WIDE_RECORDS)]
              for t in range(WIDE_TABLES)]
    ts, xs = rng.integers(0, WIDE_TABLES, WIDE_QUERIES), rng.integers(0, 2 * WIDE_RECORDS - 1, WIDE_QUERIES)
    return tables, [b"w%04d-%04d" % (int(t), int(x)) for t, x in zip(ts, xs)]


def images(entries, step=100):
    return data_image(entries), index_image(entries, step)
