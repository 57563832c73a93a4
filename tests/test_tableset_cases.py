"""The fence model of tests/tableset_cases.py on the CPU, without the library:
a fenced (query, table) pair is None under get_cases' literal SsTable::get --
for every case table of get_cases and every doctored table, over a small
universe of keys and at the caps 1, 4 and 256 -- and the hand-worked answers
of the doctored tables.  The wide order's fenced share is a property of the
input and is asserted here, so that the GPU test cannot pass with idle fences."""
import pytest

import get_cases as G
import tableset_cases as T

CAPS = (1, 4, 256)


def case_tables():
    out = [(name, G.images(e)) for name, e in G.sized_tables()]
    out += [(name, G.images(e, s)) for name, e, s in G.tie_tables()]
    out += list(G.quirk_tables().items())
    out += [("cut %d" % c, tab) for c, tab, _ in G.cut_tables()]
    return out


def universe(tables):
    """Every key of every record and index item, around() each, a few fixed ones."""
    seen, out = set(), []
    for data, index in tables:
        keys = G.btreemap(index)[0][:3] + G.btreemap(index)[0][-2:]
        f, pos, recs = T._File(data), 0, []
        while True:
            r = T.read_record(f, pos)
            if r is None:
                break
            recs.append(r[0][0])
            pos += r[1]
        for k in keys + recs[:3] + recs[98:102] + recs[-3:]:
            for c in T.around(k):
                if c not in seen:
                    seen.add(c)
                    out.append(c)
    return out + [k for k in (b"", b"\xff" * 19, b"A", b"k", b"q00100x") if k not in seen]


def holds(tables, keys, cap):
    """fenced => None; returns (pairs, fenced pairs)."""
    fenced = 0
    for data, index in tables:
        f, m = T.Fence(data, index, cap), G.btreemap(index)
        for k in keys:
            if f.fenced(k):
                fenced += 1
                assert G.table_get(data, index, k, m) is None, (k, f.low, f.high, cap)
    return len(tables) * len(keys), fenced


@pytest.mark.parametrize("cap", CAPS)
def test_fenced_pairs_are_none_on_the_case_tables(cap):
    tables = [t for _, t in case_tables()]
    pairs, fenced = holds(tables, universe(tables[::3]), cap)
    print("case tables: cap", cap, "pairs", pairs, "fenced", fenced)
    assert fenced > 0


@pytest.mark.parametrize("cap", CAPS)
def test_fenced_pairs_are_none_on_the_doctored_tables(cap):
    d = T.doctored(cap)
    tables = [t for t, _ in d.values()]
    keys = T.doctored_batch(cap)[1]
    pairs, fenced = holds(tables, keys + universe(tables), cap)
    print("doctored: cap", cap, "pairs", pairs, "fenced", fenced)
    assert fenced > 0


def test_doctored_fences_by_hand():
    d = T.doctored()
    F = {name: T.Fence(*tab) for name, (tab, _) in d.items()}
    get = lambda name, k: G.table_get(*d[name][0], k)  # noqa: E731
    # the head keys lie below key_0: no low fence, and they are found
    assert F["first item missing"].low is None and F["first item missing"].high == b"d0249"
    assert get("first item missing", b"d0050")[1] == b"val50"
    # the record at 0 lies below key_0 = d0000 at pos_0 = 0: the query for its key is Some
    assert F["low record at 0"].low is None and get("low record at 0", b"a-low")[1] == b"found-below-key0"
    # the tail's maximum is not its last record
    assert F["unsorted tail"].high == b"zz-max" and F["unsorted tail"].low == b"d0000"
    assert get("unsorted tail", b"zz-max")[1] == b"top" and get("unsorted tail", b"m-last")[1] == b"end"
    assert F["unsorted tail"].fenced(b"zz-max\x00") and not F["unsorted tail"].fenced(b"zz-max")
    # a cut last record is not visited
    assert F["cut tail"].high == b"d0248" and F["cut tail header"].high == b"d0248" and get("cut tail", b"d0249") is None
    # no record at pos_{m-1}: hi is key_{m-1}
    for name in ("last pos at end", "last pos past end", "last pos max"):
        assert F[name].high == b"d0200", name
        assert get(name, b"d0201") is None and F[name].fenced(b"d0201")
    assert F["last pos at record 5"].high == b"d0249" and get("last pos at record 5", b"d0249")[1] == b"val249"
    # caps: 7 records in the head and 9 in the tail; 4 and 4
    for cap, low, high in ((256, b"h00", b"h19"), (9, b"h00", b"h19"), (8, b"h00", None), (7, b"h00", None), (6, None, None)):
        f = T.Fence(*d["long head and tail"][0], cap)
        assert (f.low, f.high) == (low, high), cap
    for cap, low, high in ((4, b"f00", b"f07"), (3, None, None), (1, None, None)):
        f = T.Fence(*d["four and four"][0], cap)
        assert (f.low, f.high) == (low, high), cap
    # m == 0
    assert (F["no items"].low, F["no items"].high) == (None, None) and get("no items", b"d0004")[1] == b"val4"
    # ties past 8 bytes and prefixes
    f = F["ties past 8"]
    assert (f.low, f.high) == (b"TIEDKEY-aaaa", b"TIEDKEY-bbbbbbbbbbbbbbbc")
    assert f.fenced(b"TIEDKEY-aaa") and f.fenced(b"TIEDKEY-aaa\x60\xff") and f.fenced(b"TIEDKEY-") and not f.fenced(b"TIEDKEY-aaaa\x00")
    assert f.fenced(b"TIEDKEY-bbbbbbbbbbbbbbbc\x00") and not f.fenced(b"TIEDKEY-bbbbbbbbbbbbbbbc")
    f = F["prefixes"]
    assert (f.low, f.high) == (b"prefix-89", b"prefix-89abc")
    assert f.fenced(b"prefix-8") and not f.fenced(b"prefix-89a") and f.fenced(b"prefix-89abc\x00")
    # the empty key
    assert F["empty key first"].low == b"" and not F["empty key first"].fenced(b"") and F["empty key first"].fenced(b"c")
    f = F["empty key in the tail"]
    assert (f.low, f.high) == (b"k1", b"k1") and f.fenced(b"") and get("empty key in the tail", b"") is None


def test_doctored_batch_expected_values():
    """The doctored tables as one search order: the literal loop answers, and the fences leave every answer as it is."""
    tables, keys = T.doctored_batch()
    b = G.GetBatch(tables, keys)
    res = b.expected()
    assert int((res["table"] != G.NONE_TABLE).sum()) > 20
    fences = [T.Fence(d, x) for d, x in tables]
    for k, r in zip(keys, res):
        if int(r["table"]) != G.NONE_TABLE:
            assert not fences[int(r["table"])].fenced(k), k


def test_the_wide_order_is_fenced():
    tables, keys = T.wide_order()
    imgs = [T.images(t) for t in tables]
    assert (len(imgs), len(tables[0]), len(keys)) == (300, 40, 2000)
    fenced = T.count_fenced(imgs, keys)
    pairs = len(imgs) * len(keys)
    print("wide order: pairs", pairs, "fenced", fenced, "share", fenced / pairs)
    assert fenced >= 0.95 * pairs
    assert fenced == pairs - len(keys)  # every table but the key's own
    assert T.count_fenced(imgs, keys, cap=1) < fenced  # a tail of 40 records is longer than a cap of 1
    # and the answers: an even number is present, in its own table
    b = G.GetBatch(imgs, keys[:200])
    res = b.expected(fast=True, entries=tables)
    for k, r in zip(keys[:200], res):
        assert (int(r["table"]) != G.NONE_TABLE) == (int(k[-4:]) % 2 == 0)
        assert int(r["table"]) in (G.NONE_TABLE, int(k[1:5]))
