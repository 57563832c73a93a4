"""Cases and expected values for the batch SSTable decode and merge
(lsmck_sstable_decode_batch, lsmck_sstable_merge_batch).

The expected values come from two literal restatements of the reference, and
from nothing else; neither imports the library:
  * ``read_record`` / ``iterate``: the data file's iterator
    (src/sync/sstable.rs:77-90 over datafile.rs:60-83);
  * ``merge_compact_loop``: SsTable::merge_compact's loop
    (src/sync/sstable.rs:157-208), with an iteration guard that reports the
    key on which it stops advancing.
tests/test_merge_cases.py proves on the CPU what the GPU tests then rely on:
that on strictly increasing tables the loop equals "update a dict in table
order, then sort", and where it sticks.
"""
import struct

import numpy as np

GUARD = 64  # bytes of 0xAA on either side of an output
INDEX_STEP = 100  # src/sync/sstable.rs:17
TOMBSTONE = b"\x00"

WAL_CMD_DTYPE = np.dtype([("key_off", "<u8"), ("val_off", "<u8"), ("klen", "<u4"), ("vlen", "<u4"),
                          ("type", "<u4"), ("reserved", "<u4")])
SPAN_DTYPE = np.dtype([("data_off", "<u8"), ("data_len", "<u8"), ("index_off", "<u8"), ("index_len", "<u8")])


# --- layouts --------------------------------------------------------------------------
def data_image(entries):
    """datafile.rs:27-35: [u32 klen LE][u32 vlen LE][key][val] per entry."""
    return b"".join(struct.pack("<II", len(e[0]), len(e[1])) + e[0] + e[1] for e in entries)


def index_image(entries, step=INDEX_STEP):
    """sstable_index.rs:42-46, bincode fixint of BTreeMap<Vec<u8>, u64>: u64
    count, then u64 klen, key, u64 pos for every step-th entry."""
    items, pos = [], 0
    for i, e in enumerate(entries):
        if i % step == 0:
            items.append(struct.pack("<Q", len(e[0])) + e[0] + struct.pack("<Q", pos))
        pos += 8 + len(e[0]) + len(e[1])
    return struct.pack("<Q", len(items)) + b"".join(items)


# --- restatement 1: the iterator ------------------------------------------------------
class UnexpectedEof(Exception):
    pass


class _File:
    """A data file as the reference reads it: seek, then read_exact."""

    def __init__(self, image):
        self.image, self.at = bytes(image), 0

    def seek(self, pos):
        self.at = pos

    def read_exact(self, n):
        if len(self.image) - self.at < n:
            self.at = len(self.image)
            raise UnexpectedEof()
        out = self.image[self.at:self.at + n]
        self.at += n
        return out

    def read_u32(self):
        return struct.unpack("<I", self.read_exact(4))[0]


def read_record(f, pos):
    """datafile.rs:60-83: Some((pair, len)) or None on UnexpectedEof."""
    try:
        f.seek(pos)
        key_len = f.read_u32()
        val_len = f.read_u32()
        key = f.read_exact(key_len)
        val = f.read_exact(val_len)
        return (key, val), (8 + key_len + val_len) & 0xFFFFFFFF  # (u32 arithmetic)
    except UnexpectedEof:
        return None


def iterate(image):
    """sync/sstable.rs:77-90: the pairs, and the position the iterator stopped at."""
    f, pos, out = _File(image), 0, []
    while True:
        r = read_record(f, pos)
        if r is None:
            return out, pos
        out.append(r[0])
        pos += r[1]


# --- restatement 2: the merge loop ----------------------------------------------------
class Stuck(Exception):
    """The loop made an iteration that advanced nothing: ``kv`` is the winner it holds."""

    def __init__(self, kv):
        self.kv = kv
        super().__init__(f"stuck on key {kv[0]!r}")


def merge_compact_loop(tables, tombstones="continue"):
    """sync/sstable.rs:157-208 over tables given as lists of tuples (key,
    value, ...) in vector order; only [0] and [1] are looked at, so a tuple
    may carry a tag.  ``tombstones``: "continue" is the reference's line
    (:193-195), which advances nothing -- the guard raises Stuck; "drop"
    advances the winner first; "keep" writes it.  Returns what is written."""
    iterators = [iter(t) for t in tables]
    values = [next(it, None) for it in iterators]
    written, advanced = [], 0

    def nxt(i):
        nonlocal advanced
        advanced += 1
        return next(iterators[i], None)

    while True:
        before = advanced
        current_idx = None
        for i in range(len(iterators)):
            kv = values[i]
            if kv is not None:
                if current_idx is None:
                    current_idx = i
                else:
                    curr = current_idx
                    if kv[0] <= values[curr][0]:
                        current_idx = i
                    if values[curr][0] == kv[0]:
                        values[curr] = nxt(curr)
        if current_idx is None:
            break
        idx = current_idx
        kv = values[idx]
        if kv[1] == TOMBSTONE and tombstones != "keep":
            if tombstones == "drop":
                values[idx] = nxt(idx)
                continue
            if advanced == before:  # the guard: nothing moved in this iteration, nothing ever will
                raise Stuck(kv)
            continue
        written.append(kv)
        values[idx] = nxt(idx)
    return written


def dict_then_sort(tables, drop_tombstones=False):
    """What the loop is claimed to compute on strictly increasing tables."""
    d = {}
    for t in tables:
        for e in t:
            d[e[0]] = e
    return [d[k] for k in sorted(d) if not (drop_tombstones and d[k][1] == TOMBSTONE)]


# --- decode cases -----------------------------------------------------------------------
def table(m, seed=0):
    """m entries, strictly increasing keys; empty keys, empty values and a
    tombstone among them."""
    out = []
    for i in range(m):
        k = b"" if i == 0 and seed % 2 == 0 else b"k%c%07d" % (65 + seed % 26, i) + b"x" * ((i * 5 + seed) % 9)
        v = b"" if (i + seed) % 11 == 3 else bytes([(i * 31 + seed + j) % 251 for j in range((i * 7 + seed) % 19)])
        out.append((k, v))
    return out


def fixed_table(m, seed=0):
    """m entries with keys of 12 bytes: the index's items lie a fixed step apart."""
    return [(b"%c%011d" % (97 + seed % 26, i), b"v" * ((i * 5 + seed) % 17)) for i in range(m)]


DECODE_SIZES = [0, 1, 99, 100, 101, 199, 200, 201, 1000]


def damaged_indexes(entries):
    """(name, index image) for every way an index must be refused; entries: more than 200."""
    assert len(entries) > 200
    x = index_image(entries)
    k0, k1 = len(entries[0][0]), len(entries[100][0])
    pos0 = 8 + 8 + k0
    pos1 = pos0 + 8 + 8 + k1
    pos2 = pos1 + 8 + 8 + len(entries[200][0])

    def add(img, at, delta):
        v = (struct.unpack_from("<Q", img, at)[0] + delta) % 2 ** 64
        return img[:at] + struct.pack("<Q", v) + img[at + 8:]
    p1, p2 = x[pos1:pos1 + 8], x[pos2:pos2 + 8]
    return [("pos+1", add(x, pos1, 1)), ("pos-1", add(x, pos1, -1)), ("count+1", add(x, 0, 1)),
            ("count-1", add(x, 0, -1)), ("truncated", x[:-1]), ("trailing", x + b"\x00"),
            ("pos0", add(x, pos0, 8)), ("order", x[:pos1] + p2 + x[pos1 + 8:pos2] + p1 + x[pos2 + 8:]),
            ("past", add(x, pos1, len(data_image(entries)))), ("step50", index_image(entries, 50))]


class Batch:
    """Tables' images back to back in two arenas of exactly their size; the
    data arena starts with ``front`` filler bytes, so that the first table
    starts at that residue and the last one ends flush with the allocation."""

    def __init__(self, datas, indexes, front=0):
        self.datas, self.indexes = datas, indexes
        self.spans = np.zeros(len(datas), dtype=SPAN_DTYPE)
        self.spans["data_len"] = [len(d) for d in datas]
        self.spans["index_len"] = [len(x) for x in indexes]
        self.spans["data_off"] = front + np.cumsum(self.spans["data_len"]) - self.spans["data_len"]
        self.spans["index_off"] = np.cumsum(self.spans["index_len"]) - self.spans["index_len"]
        self.data = np.frombuffer(b"\xEE" * front + b"".join(datas), dtype=np.uint8)
        self.index = np.frombuffer(b"".join(indexes), dtype=np.uint8)

    def expected(self):
        """(pairs per table, tab_first, consumed) from the iterator."""
        memo = {}
        for d in self.datas:
            if d not in memo:
                memo[d] = iterate(d)
        pairs, cons = zip(*(memo[d] for d in self.datas)) if self.datas else ((), ())
        first = np.zeros(len(self.datas) + 1, dtype=np.uint64)
        first[1:] = np.cumsum([len(p) for p in pairs])
        return list(pairs), first, np.array(cons, dtype=np.uint64)


def through_arena(arena, ents):
    a = arena.tobytes() if hasattr(arena, "tobytes") else bytes(arena)
    return [(a[ko:ko + kl], a[vo:vo + vl]) for ko, kl, vo, vl in
            zip(ents["key_off"].tolist(), ents["klen"].tolist(), ents["val_off"].tolist(), ents["vlen"].tolist())]


# --- merge cases ------------------------------------------------------------------------
B = b"ABCDEFGHIJKLMNOPQRSTUVWX"
# keys tied through 7, 8, 9 and 16 bytes, proper prefixes at 7, 8 and 9, bytes
# of 0x80 and above, 00 01 against 01 00, lengths 0..20 and 63..65
POOL = sorted(set(
    [b"", b"\x00", b"\x00\x01", b"\x01\x00", B[:7], B[:8], B[:9], B[:7] + b"\x80", B[:8] + b"\xff", B[:8] + b"\x00",
     B[:9] + b"\x00", B[:16], B[:16] + b"a", B[:16] + b"b", B[:6] + b"\x80" * 2, B[:6] + b"\x7f" * 2, b"\xff" * 8,
     b"\xff" * 9, b"\x80", b"\x7f"] +
    [B[:n] for n in range(21)] + [b"z" * n for n in (63, 64, 65)] + [b"z" * 62 + b"\x80" + b"y" * n for n in (0, 1, 2)]))
VALUES = [TOMBSTONE, b"\x00\x00", b"\x01", b"", b"value", b"v" * 17]


def _tab(keys, tag, vals=None):
    """A sorted table over `keys`; values name the table, so a winner shows where it came from."""
    keys = sorted(set(keys))
    return [(k, vals[i % len(vals)] if vals else b"t%d-%d" % (tag, i)) for i, k in enumerate(keys)]


def merge_groups():
    """[(name, [tables])]: every group is one merge; none holds a tombstone."""
    rng = np.random.default_rng(7)
    out = [("k1", [_tab(POOL, 0)]), ("empty group", []), ("empty tables", [[], []]),
           ("identical", [_tab(POOL, 0), _tab(POOL, 1)]),
           ("disjoint", [_tab(POOL[20:], 0), _tab(POOL[:20], 1)]),
           ("interleaved", [_tab(POOL[0::2], 0), _tab(POOL[1::2], 1)]),
           ("one empty", [_tab(POOL[:9], 0), [], _tab(POOL[5:14], 2)])]
    for k in (2, 3, 4, 7):
        tabs = [_tab([POOL[j] for j in rng.choice(len(POOL), size=int(rng.integers(1, len(POOL))), replace=False)], t)
                for t in range(k)]
        out.append(("k%d" % k, tabs))
    # one key against a table of 0, 1, 2, 3 or 2^k +- 1 entries: below all of it, above all, equal to its first and last
    nums = [b"n%04d" % i for i in range(1, 40)]
    for m in (0, 1, 2, 3, 5, 7, 9, 15, 17, 31, 33):
        other = nums[:m]
        for name, key in (("below", b"n0000"), ("above", b"n9999"), ("first", other[0] if m else b"n0001"),
                          ("last", other[-1] if m else b"n0002")):
            out.append(("one %s %d older" % (name, m), [_tab([key], 0), _tab(other, 1)]))
            out.append(("one %s %d newer" % (name, m), [_tab(other, 0), _tab([key], 1)]))
    return out


def tombstone_groups():
    """[(name, [tables], the key the loop sticks on or None)]."""
    t = TOMBSTONE
    pool = [_tab(POOL, 0, VALUES), _tab(POOL[::3], 1, VALUES[::-1])]
    return [
        ("wins", [[(b"a", b"1"), (b"b", b"2")], [(b"a", t), (b"c", b"3")]], b"a"),
        ("shadowed", [[(b"a", t), (b"b", b"2")], [(b"a", b"1")]], None),
        ("first key", [[(b"a", t), (b"m", b"1")], [(b"z", b"9")]], b"a"),
        ("last key", [[(b"a", b"1")], [(b"m", b"1"), (b"z", t)]], b"z"),
        ("two, the later table's first", [[(b"b", t)], [(b"a", t)]], b"a"),
        ("alone", [[(b"k", t)]], b"k"),
        ("not a tombstone", [[(b"a", b"\x00\x00"), (b"b", b"\x01"), (b"c", b"")]], None),
        ("wins in the middle of three", [[(b"b", b"1")], [(b"a", b"0"), (b"b", t)], [(b"c", b"2")]], b"b"),
        ("shadowed twice", [[(b"b", t)], [(b"b", t)], [(b"b", b"v")]], None),
        ("pool", pool, next(e[0] for e in dict_then_sort(pool) if e[1] == t)),
    ]


class MergeBatch:
    """Groups of tables as one batch: the tables' data images back to back in
    one arena of exactly its size (keys = vals = the arena), the entries that
    name them, tab_first and group_first."""

    def __init__(self, groups):
        self.groups = groups
        tables = [t for g in groups for t in g]
        self.arena = np.frombuffer(b"".join(data_image(t) for t in tables), dtype=np.uint8)
        n = sum(len(t) for t in tables)
        self.ents = np.zeros(n, dtype=WAL_CMD_DTYPE)
        pos = i = 0
        for t in tables:
            for k, v in t:
                self.ents[i] = (pos + 8, pos + 8 + len(k), len(k), len(v), 1, 0)
                pos += 8 + len(k) + len(v)
                i += 1
        self.tab_first = np.zeros(len(tables) + 1, dtype=np.uint64)
        self.tab_first[1:] = np.cumsum([len(t) for t in tables])
        self.group_first = np.zeros(len(groups) + 1, dtype=np.uint64)
        self.group_first[1:] = np.cumsum([len(g) for g in groups])

    def expected(self, tombstones):
        """The loop's output per group with every entry tagged by its index in
        ents: (pairs, src, out_first), or the tagged winner the first group
        that sticks holds.  tombstones: "continue", "drop" or "keep"."""
        pairs, src, first, i = [], [], [0], 0
        for g in self.groups:
            tagged = []
            for t in g:
                tagged.append([(k, v, i + j) for j, (k, v) in enumerate(t)])
                i += len(t)
            try:
                w = merge_compact_loop(tagged, tombstones)
            except Stuck as s:
                return s.kv
            pairs += [(k, v) for k, v, _ in w]
            src += [tag for _, _, tag in w]
            first.append(len(pairs))
        return pairs, src, np.array(first, dtype=np.uint64)
