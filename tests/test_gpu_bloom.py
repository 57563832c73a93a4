"""An opened table set's resident bloom filters ("bloom_bits") on the GPU.  No
result of any call may differ: res, out_off and out of a set opened with
filters equal the cases modules' expected values and the same set opened at
"bloom_bits" 0, byte for byte, over every batch tests/test_gpu_tableset.py
runs, with the outputs between 0xAA guards.  The counts -- the tables with a
filter, their keys, the pairs the filters drop -- are the model's
(tests/bloom_cases.py, proven on the CPU by tests/test_bloom_cases.py),
exactly."""
import contextlib

import numpy as np
import pytest

import bloom_cases as B
import dbget_cases as D
import get_cases as G
import merge_cases as M
import tableset_cases as T
from lsm_storage_engine_amd import _lib, db, sstable, wal
from test_gpu_db_get import Dev, all_queries, gather_batch, inside
from test_gpu_tableset import WAYS, as_db, open_set, set_get

pytestmark = pytest.mark.gpu
DD = (("device", "device"),)
COUNTS = ("probed", "walked", "fenced", "bloomed")


@contextlib.contextmanager
def options(ctx, bloom_bits=0, fence_walk_cap=256):
    ctx.set_option("bloom_bits", bloom_bits)
    ctx.set_option("fence_walk_cap", fence_walk_cap)
    try:
        yield
    finally:
        ctx.set_option("bloom_bits", 0)
        ctx.set_option("fence_walk_cap", 256)


@contextlib.contextmanager
def opened(ctx, b, bits, how="device", cap=256, spans=None):
    """The batch's tables as a set opened at ``bits`` per key; the option is back at 0 while the set is used."""
    d = Dev(ctx)
    try:
        with options(ctx, bits, cap):
            ts = open_set(ctx, d, b, how, spans=spans)
        with ts:
            yield ts
    finally:
        d.free()


def identical(ctx, b, want=None, bits=12, ways=DD, residue=0, spans=None, cap=256):
    """The set at ``bits`` and at 0: both answer ``want``, byte for byte, between intact guards."""
    want = b.expected() if want is None else want
    b.expected_out = want[2]
    stats = {}
    for nbits in (0, bits):
        for how in sorted(set(o for o, _ in ways)):
            with opened(ctx, b, nbits, how, cap, spans) as ts:
                stats[nbits] = {k: ts.stat(k) for k in ("bloom_tables", "bloom_keys", "bloom_bytes", "resident_bytes")}
                for called in [c for o, c in ways if o == how]:
                    res, off, out, ok = set_get(ctx, ts, b, called, residue=residue, want_total=len(want[2]))
                    bad = np.nonzero(res != want[0])[0]
                    assert ok, ("guards", nbits, how, called)
                    assert len(bad) == 0, (nbits, how, called, [(int(i), b.keys[i], res[i], want[0][i]) for i in bad[:5]])
                    assert res.tobytes() == want[0].tobytes() and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
                    res2, off2, out2, ok = set_get(ctx, ts, b, called, values=False)  # out_off == NULL
                    assert ok and res2.tobytes() == want[0].tobytes() and len(off2) == 0 and len(out2) == 0
    assert stats[0]["bloom_tables"] == stats[0]["bloom_keys"] == stats[0]["bloom_bytes"] == 0
    assert stats[bits]["resident_bytes"] - stats[0]["resident_bytes"] == stats[bits]["bloom_bytes"]
    return stats[bits]


def timed(ctx, ts, b, want):
    """One timed device get: the pair counts; the results are ``want``."""
    ctx.set_option("sst_encode_time", 1)
    try:
        res, off, out, ok = set_get(ctx, ts, b, "device", want_total=len(want[2]))
        stats = {k: ctx.get_stat("tableset_" + k) for k in COUNTS + ("probe_ns",)}
    finally:
        ctx.set_option("sst_encode_time", 0)
    assert ok and res.tobytes() == want[0].tobytes() and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
    return stats


def model_stats(ts, tables, bits, cap=256):
    """The set's stats are the model's: the tables with a filter, their keys, the blocks and a descriptor per table."""
    m = B.set_stats(tables, bits, cap)
    got = {k: ts.stat(k) for k in ("bloom_tables", "bloom_keys", "bloom_bytes")}
    assert got == {"bloom_tables": m["bloom_tables"], "bloom_keys": m["bloom_keys"],
                   "bloom_bytes": 32 * m["blocks"] + 16 * len(tables)}, (got, m)
    return m


# --- 1. byte-identical -----------------------------------------------------------------
def test_dbget_cases_byte_identical(ctx):
    """precedence, six runs in front of tables, the gather's lengths, the degenerate shapes; one batch at 4 bits every way."""
    runs, tabs, keys = D.precedence()
    identical(ctx, D.DbGetBatch([D.Run(runs[0], 3, 5), D.Run(runs[1], 1, 2, one=True)], [G.images(t) for t in tabs], keys,
                                front=3, qfront=1))
    pairs = [D.run_pairs(m, 3 + j) for j, m in enumerate(D.RUN_SIZES)]
    R = [D.Run(p, 3, (21 + j) % 16, one=(3 + j) % 3 == 0) for j, p in enumerate(pairs)]
    sized = [t for _, t in G.sized_tables()][5:11]
    b = D.DbGetBatch(R, [G.images(t) for t in sized], all_queries(pairs + sized), front=2, qfront=3)
    want = b.expected()
    identical(ctx, b, want)
    identical(ctx, b, want, bits=4, ways=WAYS)
    identical(ctx, gather_batch(5), residue=5)
    identical(ctx, D.DbGetBatch(R[:2], [], keys, qfront=2))  # ntab == 0: the empty set
    identical(ctx, D.DbGetBatch([], [], keys))
    identical(ctx, D.DbGetBatch(R[:2], [G.images(t) for t in tabs], []))  # n == 0
    identical(ctx, D.DbGetBatch([D.Run([]), D.Run([])], [G.images([])], keys))  # empty sources


def test_seeded_byte_identical(ctx):
    runs, tabs, keys = D.seeded()
    b = D.DbGetBatch([D.Run(runs[0], 5, 9), D.Run(runs[1], 2, 0, one=True)], [G.images(t) for t in tabs], keys,
                     front=11, qfront=2)
    identical(ctx, b, b.expected(fast=True, entries=tabs), residue=7)
    tabs, keys = G.seeded_batch()
    b = as_db(G.GetBatch([G.images(t) for t in tabs], keys, front=5))
    s = identical(ctx, b, b.expected(fast=True, entries=tabs))
    assert s["bloom_tables"] == len(tabs)


def test_get_cases_byte_identical(ctx):
    """get_cases' sized, tie, quirk, cut and several tables with nrun == 0."""
    sized = [t for _, t in G.sized_tables()]
    batches = [G.GetBatch([G.images(t) for t in sized], all_queries(sized), front=7, qfront=3)]
    tabs = [(e, s) for _, e, s in G.tie_tables()]
    batches.append(G.GetBatch([G.images(e, s) for e, s in tabs], all_queries([e for e, _ in tabs], light=False)))
    e, Q = G.QUIRK_ENTRIES, G.quirk_tables()
    keys = [k for k, _ in e] + [b"", b"q", b"q00100x", b"q0010", b"q00150xx\x00", b"zzz"]
    batches.append(G.GetBatch(list(Q.values()), keys, front=7))
    batches.append(G.GetBatch([tab for _, tab, _ in G.cut_tables()], all_queries([G.cut_tables()[0][2]], light=False)))
    tabs, keys = G.several_tables()
    batches.append(G.GetBatch([G.images(t) for t in tabs], keys, qfront=1))
    for g in batches:
        b = as_db(g)
        want = b.expected()
        assert want[0].tobytes() == g.expected().tobytes()
        identical(ctx, b, want)


def test_doctored_and_overlapping_spans_byte_identical(ctx):
    """The doctored tables as one search order and reversed behind a run; thirty tables that read one index image."""
    tables, keys = T.doctored_batch()
    identical(ctx, D.DbGetBatch([], tables, keys, front=9, qfront=2))
    run = [(b"d0050", b"from-the-run"), (b"zz-max", M.TOMBSTONE)]
    identical(ctx, D.DbGetBatch([D.Run(run, 1, 2)], tables[::-1], keys, front=1), ways=(("device", "device"), ("host", "device")))
    ents = [(bytes([65 + i]), b"v%d" % i) for i in range(40)]
    run = [(b"B", b"from-the-run"), (b"Bx", b""), (b"zz", M.TOMBSTONE)]
    b = D.DbGetBatch([D.Run(run, 1, 2)], [G.images(ents, 1)], all_queries([ents, run], light=False))
    s = identical(ctx, b, ways=(("device", "device"), ("host", "device")), spans=np.repeat(b.spans, 30))
    assert s["bloom_tables"] == 30 and s["bloom_keys"] == 30 * (40 + 40 + 1)


# --- 2. interleaved, counts exact ------------------------------------------------------
def test_interleaved_counts(ctx):
    """4 tables of 1,000 16-byte keys 8 i + t, 4,000 queries, half absent: nothing is fenced, the filters drop the model's pairs."""
    tables, keys = B.interleaved()
    imgs = [T.images(t) for t in tables]
    b = D.DbGetBatch([], imgs, keys, front=4, qfront=1)
    want = b.expected(fast=True, entries=tables)
    model = B.count_bloomed(imgs, keys, 12)
    pairs = len(imgs) * len(keys)
    with opened(ctx, b, 0) as ts:
        plain = timed(ctx, ts, b, want)
    with opened(ctx, b, 12) as ts:
        model_stats(ts, imgs, 12)
        stats = timed(ctx, ts, b, want)
    print("interleaved: at 0", plain, "at 12", stats, "model", model)
    assert plain["fenced"] == 0 and plain["bloomed"] == 0
    assert stats["fenced"] == 0 and stats["bloomed"] == model and model >= 0.9 * (pairs - 2000)
    assert 0 < stats["probed"] <= pairs - model
    assert stats["walked"] < plain["walked"]


# --- 3. the wide order -----------------------------------------------------------------
def test_wide_order_counts(ctx):
    """300 disjoint tables: the fences drop what they dropped, the filters the model's pairs of the rest."""
    tables, keys = T.wide_order()
    imgs = [T.images(t) for t in tables]
    b = D.DbGetBatch([], imgs, keys, front=4, qfront=1)
    want = b.expected(fast=True, entries=tables)
    with opened(ctx, b, 12) as ts:
        assert ts.stat("fenced_low") == 300 and ts.stat("fenced_high") == 300
        model_stats(ts, imgs, 12)
        stats = timed(ctx, ts, b, want)
    fenced, bloomed = T.count_fenced(imgs, keys), B.count_bloomed(imgs, keys, 12)
    print("wide order:", stats, "model fenced", fenced, "bloomed", bloomed)
    assert stats["fenced"] == fenced and stats["bloomed"] == bloomed and bloomed > 0
    assert stats["probed"] <= len(imgs) * len(keys) - fenced - bloomed


# --- 4. key lengths --------------------------------------------------------------------
def test_key_lengths(ctx):
    """A key of every length 0..24 and its neighbours: the hash's tail word and length term on the device."""
    entries, keys = B.key_lengths()
    imgs = [G.images(entries, 7)]
    b = D.DbGetBatch([], imgs, keys, front=3, qfront=1)
    want = b.expected()
    for bits in (12, 64):
        model = B.count_bloomed(imgs, keys, bits)
        with opened(ctx, b, bits) as ts:
            model_stats(ts, imgs, bits)
            stats = timed(ctx, ts, b, want)
        print("key lengths: bits", bits, stats, "model", model)
        assert stats["bloomed"] == model and model > len(keys) // 2
    assert int((want[0]["table"] != G.NONE_TABLE).sum()) == 25


# --- 5. degenerate filters -------------------------------------------------------------
def test_degenerate_filters(ctx):
    """One record, m == 0, the empty table, tables above and below the cap in one set; the caps 1 and 4 on the doctored batch."""
    d = T.doctored()
    one = [(b"only", b"one")]
    imgs = [G.images(one), d["no items"][0], (b"", G._items_image([])), d["long head and tail"][0], d["four and four"][0]]
    keys = [b"", b"only", b"onlx", b"only\x00", b"d0000", b"d0004", b"d0005", b"h00", b"h07", b"h19", b"f00", b"f03", b"f07", b"g"]
    b = D.DbGetBatch([], imgs, keys, front=5, qfront=3)
    want = b.expected()
    for cap, filters in ((256, 5), (4, 3)):  # at a cap of 4: "no items" walks 5 records, the long head 7
        model = B.count_bloomed(imgs, keys, 12, cap)
        with opened(ctx, b, 12, cap=cap) as ts:
            m = model_stats(ts, imgs, 12, cap)
            stats = timed(ctx, ts, b, want)
        print("degenerate: cap", cap, stats, "model", m, model)
        assert m["bloom_tables"] == filters and stats["bloomed"] == model
        assert stats["fenced"] == T.count_fenced(imgs, keys, cap)
    f = B.Filter(*imgs[2], 12)
    assert f.valid and f.nblocks == 1 and not any(f.holds(k) for k in keys)  # the empty table drops every pair
    for cap in (1, 4):
        tables, keys = T.doctored_batch(cap)
        doc = D.DbGetBatch([], tables, keys)
        want = doc.expected()
        model = B.count_bloomed(tables, keys, 12, cap)
        with opened(ctx, doc, 12, cap=cap) as ts:
            m = model_stats(ts, tables, 12, cap)
            stats = timed(ctx, ts, doc, want)
        print("doctored: cap", cap, stats, "model", m, model)
        assert 0 < m["bloom_tables"] < len(tables) and stats["bloomed"] == model
        assert stats["fenced"] == T.count_fenced(tables, keys, cap)


# --- 6. the stride loop ----------------------------------------------------------------
def test_stride_loop(ctx):
    """65 disjoint tables x (2^20 + 3) 8-byte queries at 12 bits: more pairs
    than one pass of the grid at 16 per thread.  Table t holds the keys
    16 t + 2 i, i < 8, as 8 big-endian bytes; the expected results are a numpy
    lookup."""
    ntab, m, n = 65, 8, (1 << 20) + 3
    t = np.repeat(np.arange(ntab, dtype=np.uint64), m)
    i = np.tile(np.arange(m, dtype=np.uint64), ntab)
    rec = np.zeros((ntab * m, 20), dtype=np.uint8)
    rec[:, 0], rec[:, 4] = 8, 4
    rec[:, 8:16] = (np.uint64(16) * t + np.uint64(2) * i).astype(">u8").view(np.uint8).reshape(-1, 8)
    rec[:, 16:20] = (t * np.uint64(m) + i).astype("<u4").view(np.uint8).reshape(-1, 4)
    data = rec.ravel()
    item = np.zeros((ntab, 32), dtype=np.uint8)  # count 1, klen 8, the key, pos 0
    item[:, 0], item[:, 8] = 1, 8
    item[:, 16:24] = rec[::m, 8:16]
    index = item.ravel()
    spans = np.zeros(ntab, dtype=_lib.SSTABLE_SPAN_DTYPE)
    spans["data_len"], spans["index_len"] = 20 * m, 32
    spans["data_off"], spans["index_off"] = np.arange(ntab) * 20 * m, np.arange(ntab) * 32
    rng = np.random.default_rng(65)
    x = rng.integers(0, 16 * ntab + 16, n).astype(np.uint64)
    qkeys = x.astype(">u8").view(np.uint8)
    q = np.zeros(n, dtype=_lib.GET_QUERY_DTYPE)
    q["klen"], q["key_off"] = 8, np.arange(n, dtype=np.uint64) * np.uint64(8)
    qt, qi = x // np.uint64(16), (x % np.uint64(16)) // np.uint64(2)
    hit = (qt < ntab) & (x % np.uint64(2) == 0)
    want = np.zeros(n, dtype=_lib.GET_RESULT_DTYPE)
    want["table"] = _lib.GET_NONE
    want["table"][hit], want["vlen"][hit] = qt[hit], 4
    want["val_off"][hit] = (qt[hit] * np.uint64(m) + qi[hit]) * np.uint64(20) + np.uint64(16)
    d = Dev(ctx)
    try:
        dd, dx, ds, dqk, dq, dres = d.up(data), d.up(index), d.up(spans), d.up(qkeys), d.up(q), d.guarded(16 * n)
        with options(ctx, 12):
            ts = ctx.tableset_open(dd.ptr, dx.ptr, ds.ptr, ntab=ntab, data_bytes=data.nbytes, index_bytes=index.nbytes)
        with ts:
            assert n * ntab > (1 << 14) * 256 * 16 and ts.stat("bloom_tables") == ntab and ts.stat("bloom_keys") == ntab * 10
            assert ts.get_batch_device([], dqk.ptr, qkeys.nbytes, dq.ptr, n, dres.ptr + dres.at) == 0
            res, ok = inside(dres, 16 * n)
            res = res.view(_lib.GET_RESULT_DTYPE)
            bad = np.nonzero(res != want)[0]
            print("stride loop: pairs", n * ntab, "hits", int(hit.sum()), "mismatches", len(bad))
            assert ok and len(bad) == 0, [(int(j), int(x[j]), res[j], want[j]) for j in bad[:5]]
    finally:
        d.free()


# --- 7. runs in front, independence, the option ----------------------------------------
def test_runs_in_front_and_independence(ctx):
    """The bloomed count is taken before the winner check: two runs in front
    leave it as it is.  A second set and other calls in between leave the
    first set's answers as they are."""
    tables, keys = B.interleaved()
    imgs = [T.images(t) for t in tables]
    r0 = [(k, b"run0-%d" % j) for j, k in enumerate(sorted(set(keys[:600:3])))]
    r1 = [(k, M.TOMBSTONE if j % 2 else b"run1") for j, k in enumerate(sorted(set(keys[1:900:4])))]
    plain = D.DbGetBatch([], imgs, keys, front=4, qfront=1)
    b = D.DbGetBatch([D.Run(r0, 2, 3), D.Run(r1, 1, 0, one=True)], imgs, keys, front=4, qfront=1)
    want, pwant = b.expected(fast=True, entries=tables), plain.expected(fast=True, entries=tables)
    model = B.count_bloomed(imgs, keys, 12)
    otabs, okeys = G.seeded_batch(seed=3, ntab=24, nq=512)
    oimgs = [G.images(t) for t in otabs]
    other = as_db(G.GetBatch(oimgs, okeys))
    owant = other.expected(fast=True, entries=otabs)
    with opened(ctx, b, 12) as ts:
        first = timed(ctx, ts, plain, pwant)
        with opened(ctx, other, 5) as ts2:  # a second set with filters of its own
            assert ts2.stat("bloom_tables") == 24
            assert timed(ctx, ts2, other, owant)["bloomed"] == B.count_bloomed(oimgs, okeys, 5)
            ores = ctx.sstable_get_batch(other.data, other.index, other.spans, other.qkeys, other.q)
            assert ores.tobytes() == owant[0].tobytes()
            log = wal.CommandLog.new_in_memory()
            for i in range(2000):
                log.log(wal.Insert(b"scratch-%05d" % (i * 7 % 2000), b"v%d" % i))
            dm = wal.device_memtable(log.inner(), ctx)
            assert dm.nent == 2000
            dm.free()
            behind = timed(ctx, ts, b, want)
        again = timed(ctx, ts, plain, pwant)
    print("runs in front:", first, behind, again, "model", model)
    assert first["bloomed"] == behind["bloomed"] == again["bloomed"] == model
    assert behind["probed"] < first["probed"] and {k: first[k] for k in COUNTS} == {k: again[k] for k in COUNTS}


def test_option_values(ctx):
    """1..3, 65 and -1 are refused; 0 opens a set without filters."""
    for v in (1, 2, 3, 65, -1):
        with pytest.raises(_lib.LsmckError):
            ctx.set_option("bloom_bits", v)
    assert ctx.get_stat("bloom_bits") == 0
    for v in (4, 64, 0):
        ctx.set_option("bloom_bits", v)
        assert ctx.get_stat("bloom_bits") == v
    tables, keys = T.doctored_batch()
    b = D.DbGetBatch([], tables, keys)
    with opened(ctx, b, 0) as ts:
        assert ts.stat("bloom_tables") == 0 and ts.stat("bloom_keys") == 0 and ts.stat("bloom_bytes") == 0
        assert timed(ctx, ts, b, b.expected())["bloomed"] == 0


def test_reader_bloom_bits(ctx, tmp_path):
    """db.Reader(levels, ctx, bloom_bits): filters on its set, the option restored, db.get_many's answers."""
    l0 = [M.table(120, 0), M.table(101, 2) + [(b"zz", b"old")], [(b"kA0000003xxxxxxx", b"newest"), (b"zz", M.TOMBSTONE)]]
    metas = [[sstable._write_table(sstable.SsTableMetadata.new(str(tmp_path), 0, timestamp_ms=1000 + i),
                                   *sstable.table_bytes(sorted(t))) for i, t in enumerate(l0)]]
    mem = wal.MemTable()
    mem.insert(b"zz", b"mem")
    keys = all_queries([sorted(t) for t in l0])
    ctx.set_option("bloom_bits", 5)
    try:
        with db.Reader(metas, ctx, bloom_bits=12) as reader, db.Reader(metas, ctx) as plain:
            assert ctx.get_stat("bloom_bits") == 5
            assert reader.set.stat("bloom_tables") == 3 and plain.set.stat("bloom_tables") == 0
            assert reader.set.stat("resident_bytes") - plain.set.stat("resident_bytes") == reader.set.stat("bloom_bytes")
            for mems in ([mem], []):
                assert reader.get_many(mems, keys, internal=True) == db.get_many(mems, metas, keys, internal=True)
    finally:
        ctx.set_option("bloom_bits", 0)
