"""The bloom model of tests/bloom_cases.py on the CPU, without the library: a
key the filter does not hold is None under get_cases' literal SsTable::get --
for every case table of get_cases and every doctored table, every table key
and the keys around it, at the caps 1, 4 and 256 --, the tables whose walks
pass the cap have no filter, the hash's known answers (the same numbers stand
in tests/native/test_bloom.cpp), the false-positive rate at 12 bits per key,
and the share of the interleaved shape's pairs that the filters drop, so that
the GPU tests cannot pass with idle filters."""
import numpy as np
import pytest

import bloom_cases as B
import get_cases as G
import tableset_cases as T

CAPS = (1, 4, 256)

# key_hash(bytes(range(1, n + 1))), n = 0..24
KNOWN = [
    0x0000000000000000, 0x9E0160293A33AAF7, 0xEBD1BD6E1374CB0D, 0x4B6FB9192CB85E54,
    0x958C922B50D90CE3, 0x7DE43CC28CDD9AB5, 0xA02A6AB0FA9EC8D9, 0x06F04AC25E0D20B3,
    0x2D26208944ED5837, 0x0D1740B607B11A4C, 0x2AE626ADC758D79B, 0xEFF24E8B8F4D2C15,
    0x9BDC06C0036828C9, 0x9979B164C771CBDA, 0xCB52A57C251065F5, 0x46ED73D1CD8BD7DD,
    0xA9096F9E18B7AB22, 0x4CD22D92EB2B4D2B, 0x3348C676A1B33B7C, 0xE0DF011DDEF51775,
    0x4699E22D06EF3B92, 0xDDC87583F442E630, 0x3D288599E95F6FFD, 0xB71DE39302D90497,
    0xC45E1CC1E2E574C0,
]


def case_tables():
    out = [(name, G.images(e)) for name, e in G.sized_tables()]
    out += [(name, G.images(e, s)) for name, e, s in G.tie_tables()]
    out += list(G.quirk_tables().items())
    out += [("cut %d" % c, tab) for c, tab, _ in G.cut_tables()]
    out += [("several %d" % i, G.images(t)) for i, t in enumerate(G.several_tables()[0])]
    return out


def table_keys(data, index):
    """Every item key and every record's key of the table, in file order."""
    keys = list(G.btreemap(index)[0])
    f, pos = T._File(data), 0
    while True:
        r = T.read_record(f, pos)
        if r is None:
            return keys
        keys.append(r[0][0])
        pos += r[1]


def no_false_negative(tables, cap, bits=12, extra=()):
    """filter-negative => None, for every table key and around() of each; returns (keys asked, negatives)."""
    asked = negative = 0
    for data, index in tables:
        f, m = B.Filter(data, index, bits, cap), G.btreemap(index)
        seen = set()
        for k in table_keys(data, index) + list(extra):
            for c in T.around(k):
                if c in seen:
                    continue
                seen.add(c)
                asked += 1
                if not f.holds(c):
                    negative += 1
                    assert G.table_get(data, index, c, m) is None, (c, cap, bits)
    return asked, negative


@pytest.mark.parametrize("cap", CAPS)
def test_no_false_negative_on_the_case_tables(cap):
    asked, negative = no_false_negative([t for _, t in case_tables()], cap)
    print("case tables: cap", cap, "asked", asked, "filter-negative", negative)
    assert negative > 0


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("bits", (4, 12))
def test_no_false_negative_on_the_doctored_tables(cap, bits):
    tables = [t for t, _ in T.doctored(cap).values()]
    asked, negative = no_false_negative(tables, cap, bits, extra=T.doctored_batch(cap)[1])
    print("doctored: cap", cap, "bits", bits, "asked", asked, "filter-negative", negative)
    assert negative > 0


def test_tables_without_a_filter():
    """A walk that passes the cap leaves the table without a filter: by hand on the doctored tables."""
    d = T.doctored()
    has = lambda name, cap: B.has_filter(*d[name][0], cap)  # noqa: E731
    # 7 records before pos_0, 4 between the items, 9 from pos_{m-1}
    assert [has("long head and tail", c) for c in (256, 9, 8, 4, 1)] == [True, True, False, False, False]
    # 4 records before pos_0 = pos_1, then one walk of (pos_1, pos_1): one record, and 4 in the tail
    assert [has("four and four", c) for c in (4, 3, 1)] == [True, False, False]
    # intervals of 100 records: a cap of 256 holds, 99 does not; m == 0 walks the whole file
    assert has("unsorted tail", 256) and has("unsorted tail", 100) and not has("unsorted tail", 99)
    assert has("no items", 5) and not has("no items", 4) and has("no items no data", 1)
    # the interval with the first item missing is 100 records long, the head too
    assert has("first item missing", 100) and not has("first item missing", 99)
    # a table without a filter holds every key
    f = B.Filter(*d["no items"][0], 12, 4)
    assert not f.valid and f.holds(b"anything")
    # the empty table: no keys, one zero block, every key is dropped
    f = B.Filter(b"", G._items_image([]), 12)
    assert f.valid and (f.nkeys, f.nblocks) == (0, 1) and not f.holds(b"") and not f.holds(b"k")
    # sizes: duplicates counted -- the 3 item keys, the 250 records, and the record at 0 once more: the walk of
    # scan_range(0, pos_0 = 0) attempts it
    data, index = G.images(G.QUIRK_ENTRIES)
    f = B.Filter(data, index, 12)
    assert f.nkeys == 250 + 3 + 1 and f.nblocks == -(-254 * 12 // 256) and B.nblocks(1, 4) == 1 and B.nblocks(64, 4) == 1
    assert B.nblocks(65, 4) == 2 and B.nblocks(4, 64) == 1 and B.nblocks(5, 64) == 2


def test_hash_known_answers():
    assert [B.key_hash(B.known_key(n)) for n in range(25)] == KNOWN
    # the length enters the hash: a key and the same key zero-extended differ
    assert B.key_hash(b"abc") != B.key_hash(b"abc\x00") and B.key_hash(b"") != B.key_hash(b"\x00")
    # the benchmark's 16-byte keys differ only past byte 8
    assert B.key_hash(B.key16(8)) != B.key_hash(B.key16(9))
    assert B.mix(1) == 0x5692161D100B05E5  # splitmix64's finaliser


def hashes16(x):
    """key_hash(key16(x)) for an array of x, in numpy."""
    def mix(z):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        h = mix(np.full(len(x), (16 * 0x9E3779B97F4A7C15) & B.M64, dtype=np.uint64))
        h = mix(h ^ np.uint64(0))  # the first word: eight zero bytes
        return mix(h ^ x.astype(np.uint64).byteswap())  # the second: x big-endian, read little-endian


def test_false_positive_rate():
    """One well-formed table of 4,096 16-byte keys 8 i at 12 bits per key: for
    every t in 1..7, at most 1 % of the 2^16 absent keys 8 i + t, i < 2^16,
    pass the filter.  1 % is the reference's own BloomFilter::new(size, 0.01)."""
    m = 4096
    entries = [(B.key16(8 * i), b"v") for i in range(m)]
    data, index = G.images(entries)
    f = B.Filter(data, index, 12)
    assert f.valid and f.nkeys == m + 41 + 1 and f.nblocks == -(-(m + 42) * 12 // 256)
    words = np.zeros(8 * f.nblocks, dtype=np.uint32)
    for w, v in f.words.items():
        words[w] = v
    assert all(f.holds(k) for k, _ in entries[::97])
    for t in range(1, 8):
        x = np.uint64(8) * np.arange(1 << 16, dtype=np.uint64) + np.uint64(t)
        h = hashes16(x)
        assert int(h[5]) == B.key_hash(B.key16(int(x[5])))
        block = ((h >> np.uint64(32)) * np.uint64(f.nblocks)) >> np.uint64(32)
        lo = h & np.uint64(0xFFFFFFFF)
        passed = np.ones(len(x), dtype=bool)
        for i, s in enumerate(B.SALT):
            bit = ((lo * np.uint64(s)) & np.uint64(0xFFFFFFFF)) >> np.uint64(27)
            passed &= (words[(block * np.uint64(8) + np.uint64(i)).astype(np.int64)] >> bit.astype(np.uint32)) & 1 == 1
        rate = passed.mean()
        print("false positives at 12 bits per key, t =", t, ":", int(passed.sum()), "of", len(x), "rate", rate)
        for j in np.nonzero(passed)[0][:2]:  # the numpy form is the model's
            assert f.holds(B.key16(int(x[j])))
        assert not f.holds(B.key16(int(x[np.nonzero(~passed)[0][0]])))
        assert rate <= 0.01


def test_the_interleaved_shape_is_bloomed():
    tables, keys = B.interleaved()
    imgs = [T.images(t) for t in tables]
    assert (len(imgs), len(tables[0]), len(keys)) == (4, 1000, 4000)
    held = [set(k for k, _ in t) for t in tables]
    not_held = sum(1 for k in keys for s in held if k not in s)
    assert T.count_fenced(imgs, keys) == 0
    bloomed = B.count_bloomed(imgs, keys, 12)
    print("interleaved: pairs", 4 * len(keys), "not held", not_held, "bloomed", bloomed)
    assert bloomed >= 0.9 * not_held and not_held == 4 * 2000 + 3 * 2000
    stats = B.set_stats(imgs, 12)
    assert stats == {"bloom_tables": 4, "bloom_keys": 4 * 1011, "blocks": 4 * -(-1011 * 12 // 256)}
