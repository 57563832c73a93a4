"""lsmck_sstable_get_batch on the GPU against the cases module's expected
values (get_cases.py: the literal SsTable::get and the table loop, whose
meaning tests/test_get_cases.py proves on the CPU), bit-exact, the results
between 0xAA guards that must stay intact.  The arenas are allocated at exactly
their size.  Then the host form, the chain encode -> get and get before and
after a compaction, and sstable.get_many with and without a context."""
import numpy as np
import pytest

import get_cases as G
import merge_cases as M
from lsm_storage_engine_amd import _lib, sstable
from lsm_storage_engine_amd.device import SstGetError
from lsm_storage_engine_amd.sstable_metadata import SsTableMetadata

pytestmark = pytest.mark.gpu
AA = 0xAA
GUARD = M.GUARD


class Dev:
    """Device buffers of one test: exact-size uploads, the results filled with 0xAA between guards."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def alloc(self, nbytes):
        d = self.ctx.alloc(max(nbytes, 1))
        self.bufs.append(d)
        return d

    def up(self, a):
        d = self.alloc(a.nbytes)
        if a.nbytes:
            d.upload(a)
        return d

    def guarded(self, nbytes):
        d = self.alloc(2 * GUARD + nbytes)
        self.ctx.memset(d.ptr, AA, d.nbytes)
        return d

    def free(self):
        for d in self.bufs:
            d.free()


def device_get(ctx, b, spans=None, q=None):
    """The device form over exact-size uploads: (results, every byte outside them still 0xAA)."""
    spans = b.spans if spans is None else spans
    q = b.q if q is None else q
    d = Dev(ctx)
    try:
        dd, dx, ds, dk, dq = d.up(b.data), d.up(b.index), d.up(spans), d.up(b.qkeys), d.up(q)
        dr = d.guarded(16 * len(q))
        ctx.sync()
        try:
            ctx.sstable_get_batch_device(dd.ptr, b.data.nbytes, dx.ptr, b.index.nbytes, ds.ptr, len(spans), dk.ptr,
                                         b.qkeys.nbytes, dq.ptr, len(q), dr.ptr + GUARD)
        except SstGetError as e:
            assert (dr.download() == AA).all(), "an error writes no byte of res"
            raise e
        raw = dr.download()
        ok = (raw[:GUARD] == AA).all() and (raw[GUARD + 16 * len(q):] == AA).all()
        return raw[GUARD:GUARD + 16 * len(q)].view(_lib.GET_RESULT_DTYPE).copy(), bool(ok)
    finally:
        d.free()


def check(ctx, b, want=None):
    want = b.expected() if want is None else want
    got, ok = device_get(ctx, b)
    bad = np.nonzero(got != want)[0]
    print("get: queries", len(b.q), "tables", len(b.spans), "found", int((want["table"] != G.NONE_TABLE).sum()),
          "mismatches", len(bad))
    assert ok, "guards"
    assert len(bad) == 0, [(int(i), b.keys[i], got[i], want[i]) for i in bad[:5]]
    return got


def all_queries(tables, light=True):
    seen, out = set(), []
    for t in tables:
        for k in G.queries_for(t, light):
            if k not in seen:
                seen.add(k)
                out.append(k)
    return out


SIZED = dict(G.sized_tables())


@pytest.mark.parametrize("front", range(16))
def test_sizes_at_every_residue(ctx, front):
    """Tables of 0, 1, 99, 100, 101, 199, 200 and 201 entries -- mixed key
    lengths for even residues (the serial parse), one key length for odd ones
    (the parallel parse) -- the first at arena residue `front`, the last flush
    against the allocation's end; the order rotates.  Every present key, and
    absent keys below, between, above, prefixes, a key plus one byte, the
    empty key; the query keys end flush with qkeys."""
    kind = "fixed" if front % 2 else "mixed"
    sizes = G.SIZES[front % 8:] + G.SIZES[:front % 8]
    tables = [SIZED["%s %d" % (kind, m)] for m in sizes]
    b = G.GetBatch([G.images(t) for t in tables], all_queries(tables), front=front, qfront=front % 5)
    got = check(ctx, b)
    assert len(set(got["table"].tolist())) >= 7  # (every non-empty table answers something, and some keys nobody)


def test_key_lengths_and_ties(ctx):
    """Key lengths 0..17 and more, keys equal in their first 8 bytes, under
    indexes of every 1st, 2nd, 3rd, 7th and 100th entry: the order-key tie path
    of the lower bound; an index whose size fits one key length and whose keys
    do not have one (the parallel parse declines)."""
    for name, ents, step in G.tie_tables():
        other = [(k + b"\x01", b"o") for k, _ in ents[::3]]
        b = G.GetBatch([G.images(ents, step), G.images(sorted(other), 2)], all_queries([ents, other], light=False),
                       front=3, qfront=1)
        check(ctx, b)
    tabs = [(e, s) for _, e, s in G.tie_tables()]
    b = G.GetBatch([G.images(e, s) for e, s in tabs], all_queries([e for e, _ in tabs], light=False))
    check(ctx, b)


def test_quirks(ctx):
    """The literal quirks, each doctored table in front of the plain one: an
    exact hit returns whatever record the item points at; a position where no
    whole record fits gives None and the next table is asked; an interval of
    200 records; start >= end still reads one record."""
    e, T = G.QUIRK_ENTRIES, G.quirk_tables()
    keys = [k for k, _ in e] + [b"", b"q", b"q00100x", b"q0010", b"q00150xx\x00", b"zzz"]
    at = {k: i for i, k in enumerate(keys)}
    for name, tab in T.items():
        b = G.GetBatch([tab, T["plain"]], keys, front=7)
        got = check(ctx, b)
        vals = b.values(got)
        if name == "other record":
            assert vals[at[e[100][0]]] == b"val-5" and int(got[at[e[100][0]]]["table"]) == 0
            assert int(got[at[e[50][0]]]["table"]) == 1  # (hidden in table 0: its interval ends at record 5)
        if name.startswith("pos "):
            assert int(got[at[e[100][0]]]["table"]) == 1 and vals[at[e[100][0]]] == b"val-100"
            assert int(got[at[e[150][0]]]["table"]) == 1
        if name == "item removed":
            assert int(got[at[e[150][0]]]["table"]) == 0 and vals[at[e[150][0]]] == b"val-150"
        if name == "start past end":
            assert int(got[at[e[150][0]]]["table"]) == 0 and int(got[at[e[151][0]]]["table"]) == 1
            assert vals[at[e[100][0]]] == b"val-150" and vals[at[e[200][0]]] == b"val-100"
        # the doctored table alone: None stays None
        check(ctx, G.GetBatch([tab], keys[::3] + keys[-6:]))


def test_a_cut_last_record(ctx):
    """A data file whose last record is cut at every byte: keys before the cut are found, the cut key is not."""
    for cut, tab, ents in G.cut_tables():
        b = G.GetBatch([tab], [k for k, _ in ents] + [b"c9", b""], front=cut % 16)
        got = check(ctx, b)
        whole = cut == len(G.data_image(ents))
        assert [int(t) for t in got["table"][:5]] == [0] * 4 + [0 if whole else G.NONE_TABLE], cut


def refused(ctx, b, table=None, query=None, spans=None, q=None):
    with pytest.raises(SstGetError) as ei:
        device_get(ctx, b, spans, q)
    print("refused: bad_table", ei.value.bad_table, "bad_query", ei.value.bad_query)
    assert (ei.value.bad_table, ei.value.bad_query, ei.value.rc) == (table, query, _lib.EINVAL)


def test_refusals(ctx):
    """Each names its table or query and leaves res untouched."""
    e = G.QUIRK_ENTRIES
    data, good = G.images(e)
    keys = [e[3][0], e[150][0], b""]
    for name, x in G.refused_indexes():
        for at in range(3):
            b = G.GetBatch([(data, x if j == at else good) for j in range(3)], keys, front=at)
            refused(ctx, b, table=at)
    fe, bad = G.refused_fixed_indexes()
    fdata, fgood = G.images(fe)
    for name, x in bad:
        b = G.GetBatch([(fdata, fgood), (fdata, x), (fdata, fgood), (fdata, x)], keys)
        refused(ctx, b, table=1)
    b = G.GetBatch([(data, good)] * 3, keys)
    for field, t, value in (("data_len", 2, int(b.spans["data_len"][2]) + 1), ("data_off", 0, 2 ** 64 - 4),
                            ("index_off", 1, b.index.nbytes + 1), ("index_len", 2, 2 ** 64 - 1)):
        s = b.spans.copy()
        s[field][t] = value
        refused(ctx, b, table=t, spans=s)
    q = b.q.copy()
    q["klen"][1] += 1000
    refused(ctx, b, query=1, q=q)
    q = b.q.copy()
    q["key_off"][0] = 2 ** 64 - 1
    refused(ctx, b, query=0, q=q)
    q = b.q.copy()
    q["reserved"][2] = 1
    refused(ctx, b, query=2, q=q)
    q["reserved"][1] = 9  # tables are checked before queries
    s = b.spans.copy()
    s["data_len"][2] += 1  # (the last table: one byte past the arena)
    refused(ctx, b, table=2, spans=s, q=q)
    q = b.q.copy()
    q["key_off"][2] = 2 ** 64 - 1  # (an empty key's offset is not looked at)
    got, ok = device_get(ctx, b, q=q)
    assert ok and np.array_equal(got, b.expected())


def test_several_tables(ctx):
    """A key in tables 0 and 2, a tombstone in table 0 over a live value in
    table 1, a key in the last table only, a key in none, duplicate queries;
    n == 0; ntab == 0."""
    tabs, keys = G.several_tables()
    b = G.GetBatch([G.images(t) for t in tabs], keys, front=5, qfront=3)
    got = check(ctx, b)
    at = {k: i for i, k in reversed(list(enumerate(keys)))}
    r = got[at[b"dead"]]
    assert (int(r["table"]), int(r["vlen"]), int(r["val_off"]) >> 63) == (0, 1, 1)
    assert int(got[at[b"both"]]["table"]) == 0 and int(got[at[b"last"]]["table"]) == 3
    assert (int(got[at[b"none"]]["table"]), int(got[at[b"none"]]["val_off"])) == (G.NONE_TABLE, 0)
    assert got[at[b"both"]] == got[5] == got[4]
    none, ok = device_get(ctx, G.GetBatch([G.images(t) for t in tabs], []))
    assert ok and len(none) == 0
    got, ok = device_get(ctx, G.GetBatch([], keys))
    assert ok and (got["table"] == G.NONE_TABLE).all() and (got["val_off"] == 0).all() and (got["vlen"] == 0).all()
    assert len(ctx.sstable_get_batch(b.data, b.index, b.spans, b.qkeys, b.q[:0])) == 0


def test_overlapping_index_spans(ctx):
    """Thirty tables that read one index image: more items than the index arena's bytes suggest."""
    ents = [(bytes([65 + i]), b"v%d" % i) for i in range(40)]
    b = G.GetBatch([G.images(ents, 1)], all_queries([ents], light=False))
    spans = np.repeat(b.spans, 30)
    got, ok = device_get(ctx, b, spans=spans)
    assert ok and np.array_equal(got, b.expected())


@pytest.fixture(scope="module")
def seeded():
    tabs, keys = G.seeded_batch()
    b = G.GetBatch([G.images(t) for t in tabs], keys, front=11, qfront=2)
    return b, b.expected(fast=True, entries=tabs)


def test_seeded_batch(ctx, seeded):
    """64 tables of 1..1,000 entries over overlapping key ranges, 4,096 queries, about half present."""
    b, want = seeded
    check(ctx, b, want)
    ctx.set_option("sst_encode_time", 1)
    try:
        check(ctx, b, want)
        stats = {k: ctx.get_stat(k) for k in ("sst_get_index_ns", "sst_get_probe_ns", "sst_get_resolve_ns",
                                                "sst_get_probed", "sst_get_walked")}
        print("stats", stats)
        assert all(v > 0 for v in stats.values())
        assert stats["sst_get_walked"] <= stats["sst_get_probed"] <= len(b.q) * len(b.spans)
    finally:
        ctx.set_option("sst_encode_time", 0)


def test_host_form_equals_device_form(ctx, seeded):
    b, want = seeded
    assert np.array_equal(ctx.sstable_get_batch(b.data, b.index, b.spans, b.qkeys, b.q), want)
    assert np.array_equal(ctx.sstable_get_batch(b.data, b.index, b.spans, b.qkeys, b.q, pinned=True), want)
    tabs, keys = G.several_tables()
    s = G.GetBatch([G.images(t) for t in tabs], keys, front=1)
    assert np.array_equal(ctx.sstable_get_batch(s.data, s.index, s.spans, s.qkeys, s.q), s.expected())
    bad = s.spans.copy()
    bad["index_len"][2] -= 1
    with pytest.raises(SstGetError) as ei:
        ctx.sstable_get_batch(s.data, s.index, bad, s.qkeys, s.q)
    assert (ei.value.bad_table, ei.value.bad_query) == (2, None)
    q = s.q.copy()
    q["reserved"][4] = 1
    with pytest.raises(SstGetError) as ei:
        ctx.sstable_get_batch(s.data, s.index, s.spans, s.qkeys, q)
    assert (ei.value.bad_table, ei.value.bad_query) == (None, 4)


def test_chain_encode_get_and_get_after_a_compaction(ctx):
    """Tables written by lsmck_sstable_encode_batch in the same context are
    queried where they lie; after lsmck_sstable_merge_batch with
    LSMCK_MERGE_KEEP_TOMBSTONES and an encode, a get over the one merged table
    equals the get over the old tables, newest first, for every key of the old
    tables and a set of absent ones: the property a compaction must keep."""
    tom = M.TOMBSTONE
    old = [M.table(250, 0), M.table(130, 2) + [(b"zz", b"live")],
           sorted(M.table(300, 0)[::2] + [(b"kA0000003xxxxxxx!", tom), (b"zz", tom)]), M.table(101, 6)]  # oldest first
    keys = all_queries(old, light=True)
    kb = G.GetBatch([], keys, qfront=1)
    akeys, avals, ents, first = sstable.batch_arrays(old)
    files = [sstable.table_bytes(t) for t in old]
    db, ib, ntab = sum(len(f[0]) for f in files), sum(len(f[1]) for f in files), len(old)
    d = Dev(ctx)
    try:
        dk, dv, de = d.up(akeys), d.up(avals), d.up(ents)
        dd, dx, ds, dsha = d.alloc(db), d.alloc(ib), d.alloc(32 * ntab), d.alloc(64 * ntab)
        assert ctx.sstable_encode_batch_device(dk.ptr, akeys.nbytes, dv.ptr, avals.nbytes, de.ptr, len(ents), first, dd.ptr,
                                               db, dx.ptr, ib, ds.ptr, dsha.ptr, dsha.ptr + 32 * ntab) == (db, ib)
        spans = ds.download(_lib.SSTABLE_SPAN_DTYPE, ntab)
        newest_first = np.ascontiguousarray(spans[::-1])
        dsr, dqk, dq = d.up(newest_first), d.up(kb.qkeys), d.up(kb.q)
        r_old, r_new = d.guarded(16 * len(keys)), d.guarded(16 * len(keys))
        ctx.sstable_get_batch_device(dd.ptr, db, dx.ptr, ib, dsr.ptr, ntab, dqk.ptr, kb.qkeys.nbytes, dq.ptr, len(keys),
                                     r_old.ptr + GUARD)
        arena = dd.download(np.uint8, db)
        assert arena.tobytes() == b"".join(f[0] for f in files)
        want = G.GetBatch(files[::-1], keys, qfront=1)
        got_old = r_old.download()[GUARD:GUARD + 16 * len(keys)].view(_lib.GET_RESULT_DTYPE)
        assert np.array_equal(got_old["table"], want.expected()["table"])
        # (the encode lays the tables out oldest first, the expected arena newest first: compare values)
        vals_old = [(int(r["table"]), arena[(int(r["val_off"]) & (2 ** 63 - 1)):][:int(r["vlen"])].tobytes()
                     if int(r["table"]) != G.NONE_TABLE else None, int(r["val_off"]) >> 63) for r in got_old]
        exp = want.expected()
        assert [v[1] for v in vals_old] == want.values(exp) and [v[2] for v in vals_old] == (exp["val_off"] >> np.uint64(63)).tolist()
        # the compaction: decode, merge (keep), encode -- one table
        cap = db // 8
        dents, dout = d.alloc(32 * cap), d.alloc(32 * cap)
        nent, tf = ctx.sstable_decode_batch_device(dd.ptr, db, dx.ptr, ib, ds.ptr, ntab, dents.ptr, cap)
        nout, of = ctx.sstable_merge_batch_device(dd.ptr, db, dd.ptr, db, dents.ptr, nent, tf, [0, ntab], dout.ptr, cap,
                                                  tombstones="keep")
        merged = sstable.table_bytes(M.merge_compact_loop(old, "keep"))
        ndb, nib = len(merged[0]), len(merged[1])
        nd, nx, nsp, nsha = d.alloc(ndb), d.alloc(nib), d.alloc(32), d.alloc(64)
        assert ctx.sstable_encode_batch_device(dd.ptr, db, dd.ptr, db, dout.ptr, nout, of, nd.ptr, ndb, nx.ptr, nib,
                                               nsp.ptr, nsha.ptr, nsha.ptr + 32) == (ndb, nib)
        ctx.sstable_get_batch_device(nd.ptr, ndb, nx.ptr, nib, nsp.ptr, 1, dqk.ptr, kb.qkeys.nbytes, dq.ptr, len(keys),
                                     r_new.ptr + GUARD)
        raw = r_new.download()
        assert (raw[:GUARD] == AA).all() and (raw[GUARD + 16 * len(keys):] == AA).all()
        got_new = raw[GUARD:GUARD + 16 * len(keys)].view(_lib.GET_RESULT_DTYPE)
        narena = nd.download(np.uint8, ndb)
        vals_new = [(narena[(int(r["val_off"]) & (2 ** 63 - 1)):][:int(r["vlen"])].tobytes()
                     if int(r["table"]) != G.NONE_TABLE else None, int(r["val_off"]) >> 63) for r in got_new]
        print("compaction: keys", len(keys), "found before", sum(v[1] is not None for v in vals_old), "after",
              sum(v[0] is not None for v in vals_new))
        assert vals_new == [(v[1], v[2]) for v in vals_old]
        d_all = {}
        for t in old:
            d_all.update(t)
        assert [v[0] for v in vals_new] == [d_all.get(k) for k in keys]
        assert np.array_equal(got_new, G.GetBatch([merged], keys, qfront=1).expected())
    finally:
        d.free()


def test_get_many_files(ctx, tmp_path):
    """sstable.get_many with and without a context, on files: levels in the
    reference's vector order, each asked newest first."""
    tom = M.TOMBSTONE
    l0 = [M.table(120, 0), M.table(101, 2) + [(b"zz", b"old")], [(b"kA0000003xxxxxxx", b"newest"), (b"zz", tom)]]
    l1 = [M.table(250, 0), [(b"only-l1", b"deep"), (b"zz", b"l1")]]
    metas = [[sstable._write_table(SsTableMetadata.new(str(tmp_path), lvl, timestamp_ms=1000 * lvl + i),
                                   *sstable.table_bytes(sorted(t))) for i, t in enumerate(level)]
             for lvl, level in enumerate((l0, [], l1))]
    keys = all_queries([sorted(t) for t in l0 + l1])
    host = sstable.get_many(metas, keys)
    dev = sstable.get_many(metas, keys, ctx)
    assert host == dev
    order = [sorted(t) for t in l0[::-1] + l1[::-1]]
    want = G.GetBatch([G.images(t) for t in order], keys)
    exp = [sstable.TOMBSTONE_HIT if v == tom else v for v in want.values(want.expected())]
    assert dev == exp
    at = {k: i for i, k in enumerate(keys)}
    assert dev[at[b"zz"]] is sstable.TOMBSTONE_HIT and dev[at[b"kA0000003xxxxxxx"]] == b"newest"
    assert dev[at[b"only-l1"]] == b"deep" and dev[at[b"zz\x00"]] is None
    assert sstable.get_many([], [b"a"], ctx) == [None] and sstable.get_many(metas, [], ctx) == []
