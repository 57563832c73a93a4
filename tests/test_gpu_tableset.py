"""lsmck_tableset_open / lsmck_tableset_get_batch on the GPU.  The yardstick is
lsmck_db_get_batch on the same inputs (tests/test_gpu_db_get.py's device_get)
and the cases modules' expected values: res, out_off and out from a set must
equal both, byte for byte, for sets opened from device and from host arrays and
gets called both ways.  Device uploads are exact-size allocations, the outputs
lie between 0xAA guards, and after a refused call every byte is still 0xAA.
The fenced counts are the model's (tests/tableset_cases.py, proven on the CPU
by tests/test_tableset_cases.py), exactly."""
import numpy as np
import pytest

import dbget_cases as D
import get_cases as G
import merge_cases as M
import tableset_cases as T
from lsm_storage_engine_amd import _lib, db, sstable, wal
from lsm_storage_engine_amd.device import Context, DbGetError, SstGetError
from test_gpu_db_get import AA, Dev, all_queries, device_get, gather_batch, inside

pytestmark = pytest.mark.gpu
WAYS = [("device", "device"), ("device", "host"), ("host", "device"), ("host", "host")]


def open_set(ctx, d, b, how, spans=None):
    """The batch's tables as a set: from exact-size device uploads (kept in d), or from the host arrays."""
    spans = b.spans if spans is None else spans
    if how == "host":
        return ctx.tableset_open(b.data, b.index, spans)
    dd, dx, ds = d.up(b.data), d.up(b.index), d.up(spans)
    ctx.sync()
    return ctx.tableset_open(dd.ptr, dx.ptr, ds.ptr, ntab=len(spans), data_bytes=b.data.nbytes, index_bytes=b.index.nbytes)


def set_get(ctx, ts, b, how, values=True, residue=0, out_cap=None, ents=None, q=None, want_total=0, caller=None):
    """One get on the set: (res, out_off, out, every guard byte still 0xAA)."""
    q = b.q if q is None else q
    n = len(q)
    if how == "host":
        runs = [(r.keys, r.vals, r.ents if ents is None else ents[j]) for j, r in enumerate(b.runs)]
        res, off, out = ts.get_batch(runs, b.qkeys, q, values=values)
        return (res, off, out, True) if values else (res, np.zeros(0, np.uint64), np.zeros(0, np.uint8), True)
    want_total = want_total if out_cap is None else out_cap
    d = Dev(ctx)
    try:
        desc = np.zeros(len(b.runs), dtype=_lib.GET_RUN_DTYPE)
        for r, run in enumerate(b.runs):
            e = run.ents if ents is None else ents[r]
            dk = d.up(run.keys)
            dv = dk if run.vals is run.keys else d.up(run.vals)
            desc[r] = (dk.ptr, run.keys.nbytes, dv.ptr, run.vals.nbytes, d.up(e).ptr, len(e))
        dqk, dq = d.up(b.qkeys), d.up(q)
        dres, doff, dout = d.guarded(16 * n), d.guarded(8 * (n + 1)), d.guarded(want_total, residue)
        ctx.sync()
        args = (desc, dqk.ptr, b.qkeys.nbytes, dq.ptr, n, dres.ptr + dres.at)
        try:
            if values:
                total = ts.get_batch_device(*args, dout.ptr + dout.at, want_total, doff.ptr + doff.at, ctx=caller)
            else:
                total = ts.get_batch_device(*args, ctx=caller)
        except DbGetError as e:
            for x in (dres, doff, dout):
                assert (x.download() == AA).all(), "an error writes no byte of res, out_off or out"
            raise e
        res, ok1 = inside(dres, 16 * n)
        off, ok2 = inside(doff, 8 * (n + 1) if values else 0)
        out, ok3 = inside(dout, total)
        return res.view(_lib.GET_RESULT_DTYPE), off.view(np.uint64), out, ok1 and ok2 and ok3
    finally:
        d.free()


def check(ctx, b, want=None, ways=WAYS, yard=True, residue=0):
    """Sets opened and called every way against the expected values and against lsmck_db_get_batch."""
    want = b.expected() if want is None else want
    b.expected_out = want[2]
    if yard:
        res, off, out, ok = device_get(ctx, b, residue=residue)
        assert ok and res.tobytes() == want[0].tobytes() and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
    for opened in sorted(set(o for o, _ in ways)):
        d = Dev(ctx)
        try:
            with open_set(ctx, d, b, opened) as ts:
                assert ts.stat("tables") == len(b.spans)
                for called in [c for o, c in ways if o == opened]:
                    res, off, out, ok = set_get(ctx, ts, b, called, residue=residue, want_total=len(want[2]))
                    bad = np.nonzero(res != want[0])[0]
                    assert ok, ("guards", opened, called)
                    assert len(bad) == 0, (opened, called, [(int(i), b.keys[i], res[i], want[0][i]) for i in bad[:5]])
                    assert res.tobytes() == want[0].tobytes() and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
                    res2, off2, out2, ok = set_get(ctx, ts, b, called, values=False)  # out_off == NULL
                    assert ok and res2.tobytes() == want[0].tobytes() and len(off2) == 0 and len(out2) == 0
        finally:
            d.free()


def as_db(g):
    return D.DbGetBatch([], g.tables, g.keys, front=int(g.spans["data_off"][0]) if len(g.spans) else 0,
                        qfront=int(g.q["key_off"][0]) if len(g.q) else 0)


def test_dbget_cases_byte_identical(ctx):
    """precedence, six runs in front of tables, the gather's lengths, the degenerate shapes."""
    runs, tabs, keys = D.precedence()
    check(ctx, D.DbGetBatch([D.Run(runs[0], 3, 5), D.Run(runs[1], 1, 2, one=True)], [G.images(t) for t in tabs], keys,
                            front=3, qfront=1))
    pairs = [D.run_pairs(m, 3 + j) for j, m in enumerate(D.RUN_SIZES)]
    R = [D.Run(p, 3, (21 + j) % 16, one=(3 + j) % 3 == 0) for j, p in enumerate(pairs)]
    sized = [t for _, t in G.sized_tables()][5:11]
    check(ctx, D.DbGetBatch(R, [G.images(t) for t in sized], all_queries(pairs + sized), front=2, qfront=3))
    check(ctx, gather_batch(5), residue=5)
    check(ctx, D.DbGetBatch(R[:2], [], keys, qfront=2))  # ntab == 0: the empty set
    check(ctx, D.DbGetBatch([], [], keys))
    check(ctx, D.DbGetBatch(R[:2], [G.images(t) for t in tabs], []))  # n == 0
    check(ctx, D.DbGetBatch([D.Run([]), D.Run([])], [G.images([])], keys))  # empty sources


def test_dbget_seeded_byte_identical(ctx):
    runs, tabs, keys = D.seeded()
    b = D.DbGetBatch([D.Run(runs[0], 5, 9), D.Run(runs[1], 2, 0, one=True)], [G.images(t) for t in tabs], keys,
                     front=11, qfront=2)
    check(ctx, b, b.expected(fast=True, entries=tabs), residue=7)


def test_get_cases_byte_identical(ctx):
    """get_cases' sized, tie, quirk, cut and several tables with nrun == 0: also lsmck_sstable_get_batch's expected results."""
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
        check(ctx, b, want)


def test_get_cases_seeded_byte_identical(ctx):
    tabs, keys = G.seeded_batch()
    g = G.GetBatch([G.images(t) for t in tabs], keys, front=5)
    b = as_db(g)
    check(ctx, b, b.expected(fast=True, entries=tabs), ways=[("device", "device"), ("host", "host")])


def test_doctored_tables_byte_identical(ctx):
    """The doctored tables of tableset_cases as one search order, and each alone behind a run."""
    tables, keys = T.doctored_batch()
    check(ctx, D.DbGetBatch([], tables, keys, front=9, qfront=2))
    run = [(b"d0050", b"from-the-run"), (b"zz-max", M.TOMBSTONE)]
    check(ctx, D.DbGetBatch([D.Run(run, 1, 2)], tables[::-1], keys, front=1), ways=[("device", "device"), ("host", "device")])
    d = Dev(ctx)
    try:
        with open_set(ctx, d, D.DbGetBatch([], tables, keys), "device") as ts:
            assert ts.stat("tables") == len(tables) and ts.stat("resident_bytes") > 0
            fences = [T.Fence(*t) for t in tables]
            assert ts.stat("fenced_low") == sum(f.low is not None for f in fences)
            assert ts.stat("fenced_high") == sum(f.high is not None for f in fences)
            assert ts.stat("items") == sum(len(G.btreemap(x)[0]) for _, x in tables)
    finally:
        d.free()


def test_overlapping_index_spans(ctx):
    """Thirty tables that read one index image: the item arrays grow at open and the passes run again."""
    ents = [(bytes([65 + i]), b"v%d" % i) for i in range(40)]
    run = [(b"B", b"from-the-run"), (b"Bx", b""), (b"zz", M.TOMBSTONE)]
    b = D.DbGetBatch([D.Run(run, 1, 2)], [G.images(ents, 1)], all_queries([ents, run], light=False))
    want = b.expected()
    for how in ("device", "host"):
        d = Dev(ctx)
        try:
            with open_set(ctx, d, b, how, spans=np.repeat(b.spans, 30)) as ts:
                assert ts.stat("tables") == 30 and ts.stat("items") == 30 * 40
                res, off, out, ok = set_get(ctx, ts, b, "device", want_total=len(want[2]))
                assert ok and np.array_equal(res, want[0]) and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
        finally:
            d.free()


def test_refusals(ctx):
    """open names the first bad table and retains nothing; a get names the run
    entry, then the query, and leaves res, out_off and out untouched."""
    e = G.QUIRK_ENTRIES
    data, good = G.images(e)
    for name, bad_x in G.refused_indexes()[:6] + G.refused_fixed_indexes()[1][:2]:
        g = G.GetBatch([(data, good), (data, bad_x), (data, bad_x)], [e[3][0]])
        for how in ("device", "host"):
            d = Dev(ctx)
            try:
                with pytest.raises(SstGetError) as ei:
                    open_set(ctx, d, g, how)
                assert (ei.value.bad_table, ei.value.rc) == (1, _lib.EINVAL), name
            finally:
                d.free()
    spans = G.GetBatch([(data, good)] * 3, []).spans
    spans["data_len"][2] += 1
    with pytest.raises(SstGetError) as ei:
        ctx.tableset_open(np.frombuffer(data * 3, np.uint8), np.frombuffer(good * 3, np.uint8), spans)
    assert ei.value.bad_table == 2
    p0, p1 = D.run_pairs(10, 0), D.run_pairs(12, 2)
    b = D.DbGetBatch([D.Run(p0, 2, 3), D.Run(p1, 1, 0, one=True)], [(data, good)] * 2, [e[3][0], p0[4][0], b""])
    want = b.expected()
    d = Dev(ctx)
    try:
        with open_set(ctx, d, b, "device") as ts:
            def refused(run=None, query=None, **kw):
                with pytest.raises(DbGetError) as ei:
                    set_get(ctx, ts, b, "device", want_total=64, **kw)
                assert (ei.value.bad_run_entry, ei.value.bad_table, ei.value.bad_query, ei.value.rc) == \
                    (run, None, query, _lib.EINVAL)
            ents = [r.ents.copy() for r in b.runs]
            ents[1][4] = ents[1][3]
            refused(run=10 + 4, ents=ents)  # equal adjacent keys
            q = b.q.copy()
            q["reserved"][2] = 1
            refused(run=10 + 4, ents=ents, q=q)  # the run entry before the query
            refused(query=2, q=q)
            refused(query=2, q=q, values=False)
            q = b.q.copy()
            q["key_off"][1] = b.qkeys.nbytes
            refused(query=1, q=q)
            with pytest.raises(DbGetError) as ei:
                set_get(ctx, ts, b, "device", out_cap=len(want[2]) - 1)
            assert (ei.value.rc, ei.value.needed) == (_lib.ENOSPC, len(want[2]))
            with pytest.raises(DbGetError):  # the host form refuses the same way
                set_get(ctx, ts, b, "host", ents=ents)
            res, off, out, ok = set_get(ctx, ts, b, "device", want_total=len(want[2]))  # and the set still answers
            assert ok and np.array_equal(res, want[0]) and np.array_equal(out, want[2])
    finally:
        d.free()


def test_scratch_independence(ctx):
    """Two gets on one set with an unrelated lsmck_sstable_get_batch over other
    tables and a lsmck_memtable_build in between: a set that aliased the
    context's scratch would answer from the other tables' items."""
    runs, tabs, keys = D.seeded()
    b = D.DbGetBatch([D.Run(runs[0], 5, 9)], [G.images(t) for t in tabs], keys, front=11, qfront=2)
    want = b.expected(fast=True, entries=tabs)
    otabs, okeys = G.seeded_batch(seed=3, ntab=24, nq=512)
    other = G.GetBatch([G.images(t) for t in otabs], okeys)
    log = wal.CommandLog.new_in_memory()
    for i in range(3000):
        log.log(wal.Insert(b"scratch-%05d" % (i * 7 % 3000), b"v%d" % i))
    for how in ("device", "host"):
        d = Dev(ctx)
        try:
            with open_set(ctx, d, b, how) as ts:
                first = set_get(ctx, ts, b, "device", want_total=len(want[2]))
                ores = ctx.sstable_get_batch(other.data, other.index, other.spans, other.qkeys, other.q)
                assert int((ores["table"] != G.NONE_TABLE).sum()) > 100
                dm = wal.device_memtable(log.inner(), ctx)
                assert dm.nent == 3000
                dm.free()
                second = set_get(ctx, ts, b, "device", want_total=len(want[2]))
                third = set_get(ctx, ts, b, "host")
                for got in (first, second, third):
                    assert got[3] and got[0].tobytes() == want[0].tobytes()
                    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        finally:
            d.free()


def test_host_opened_set_owns_its_copies(ctx):
    """The caller's arrays are zeroed after open: the set answers from its own device copies."""
    runs, tabs, keys = D.seeded()
    b = D.DbGetBatch([], [G.images(t) for t in tabs], keys, front=3)
    want = b.expected(fast=True, entries=tabs)
    data, index, spans = b.data.copy(), b.index.copy(), b.spans.copy()
    with ctx.tableset_open(data, index, spans) as ts:
        data[:], index[:], spans[:] = 0, 0, 0
        assert ts.stat("resident_bytes") >= b.data.nbytes + b.index.nbytes
        for how in ("host", "device"):
            res, off, out, ok = set_get(ctx, ts, b, how, want_total=len(want[2]))
            assert ok and res.tobytes() == want[0].tobytes() and np.array_equal(out, want[2])


@pytest.fixture(scope="module")
def wide():
    tables, keys = T.wide_order()
    imgs = [T.images(t) for t in tables]
    b = D.DbGetBatch([], imgs, keys, front=4, qfront=1)
    return b, b.expected(fast=True, entries=tables), imgs


def timed_get(ctx, ts, b, want):
    ctx.set_option("sst_encode_time", 1)
    try:
        res, off, out, ok = set_get(ctx, ts, b, "device", want_total=len(want[2]))
        stats = {k: ctx.get_stat("tableset_" + k) for k in ("probed", "walked", "fenced", "probe_ns", "resolve_ns", "gather_ns")}
    finally:
        ctx.set_option("sst_encode_time", 0)
    assert ok and res.tobytes() == want[0].tobytes() and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
    return stats


def test_wide_order_fenced_count(ctx, wide):
    """300 disjoint tables, 2,000 queries: the fences drop exactly the model's pairs."""
    b, want, imgs = wide
    model = T.count_fenced(imgs, b.keys)
    d = Dev(ctx)
    try:
        with open_set(ctx, d, b, "device") as ts:
            assert ts.stat("fenced_low") == 300 and ts.stat("fenced_high") == 300 and ts.stat("items") == 300
            stats = timed_get(ctx, ts, b, want)
            print("wide order:", stats, "model", model)
            assert stats["fenced"] == model and model >= 0.95 * len(imgs) * len(b.keys)
            assert 0 < stats["probed"] <= len(imgs) * len(b.keys) - model and stats["probe_ns"] > 0
    finally:
        d.free()


@pytest.mark.parametrize("cap", [1, 4])
def test_fence_walk_cap(ctx, wide, cap):
    """A smaller cap: the same results from fewer fences, the model's count."""
    b, want, imgs = wide
    tables, keys = T.doctored_batch(cap)
    doc = D.DbGetBatch([], tables, keys)
    ctx.set_option("fence_walk_cap", cap)
    try:
        for batch, w, tabs in ((b, want, imgs), (doc, doc.expected(), tables)):
            model, full = T.count_fenced(tabs, batch.keys, cap), T.count_fenced(tabs, batch.keys)
            fences = [T.Fence(dd, x, cap) for dd, x in tabs]
            d = Dev(ctx)
            try:
                with open_set(ctx, d, batch, "device") as ts:
                    assert ts.stat("fenced_low") == sum(f.low is not None for f in fences)
                    assert ts.stat("fenced_high") == sum(f.high is not None for f in fences)
                    stats = timed_get(ctx, ts, batch, w)
                    print("cap", cap, stats, "model", model, "at 256", full)
                    assert stats["fenced"] == model and model < full
            finally:
                d.free()
    finally:
        ctx.set_option("fence_walk_cap", 256)
    with pytest.raises(_lib.LsmckError):
        ctx.set_option("fence_walk_cap", 0)


def test_stride_loop(ctx):
    """257 disjoint tables x (2^20 + 3) 8-byte queries: more pairs than one pass
    of the grid's 2^20 workgroups.  Table t holds the keys 16 t + 2 i, i < 8, as
    8 big-endian bytes; the expected results are a numpy lookup."""
    ntab, m, n = 257, 8, (1 << 20) + 3
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
    rng = np.random.default_rng(257)
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
        with ctx.tableset_open(dd.ptr, dx.ptr, ds.ptr, ntab=ntab, data_bytes=data.nbytes, index_bytes=index.nbytes) as ts:
            assert n * ntab > (1 << 20) * 256 and ts.stat("fenced_high") == ntab
            assert ts.get_batch_device([], dqk.ptr, qkeys.nbytes, dq.ptr, n, dres.ptr + dres.at) == 0
            res, ok = inside(dres, 16 * n)
            res = res.view(_lib.GET_RESULT_DTYPE)
            bad = np.nonzero(res != want)[0]
            print("stride loop: pairs", n * ntab, "hits", int(hit.sum()), "mismatches", len(bad))
            assert ok and len(bad) == 0, [(int(j), int(x[j]), res[j], want[j]) for j in bad[:5]]
    finally:
        d.free()


def test_another_context_is_refused(ctx):
    runs, tabs, keys = D.precedence()
    b = D.DbGetBatch([D.Run(runs[0], 3, 5)], [G.images(t) for t in tabs], keys)
    want = b.expected()
    other = Context(0)
    try:
        with ctx.tableset_open(b.data, b.index, b.spans) as ts:
            with pytest.raises(DbGetError) as ei:
                set_get(other, ts, b, "device", want_total=len(want[2]), caller=other)
            assert ei.value.rc == _lib.EINVAL and "another context" in str(ei.value)
            res, off, out, ok = set_get(ctx, ts, b, "device", want_total=len(want[2]))
            assert ok and np.array_equal(res, want[0]) and np.array_equal(out, want[2])
    finally:
        other.close()


def test_reader_equals_get_many(ctx, tmp_path):
    """db.Reader over files: db.get_many's answers, with and without memtables, call after call."""
    l0 = [M.table(120, 0), M.table(101, 2) + [(b"zz", b"old")], [(b"kA0000003xxxxxxx", b"newest"), (b"zz", M.TOMBSTONE)]]
    l1 = [M.table(250, 0), [(b"only-l1", b"deep"), (b"zz", b"l1")]]
    metas = [[sstable._write_table(sstable.SsTableMetadata.new(str(tmp_path), lvl, timestamp_ms=1000 * lvl + i),
                                   *sstable.table_bytes(sorted(t))) for i, t in enumerate(level)]
             for lvl, level in enumerate((l0, [], l1))]
    mem = wal.MemTable()
    mem.insert(b"zz", b"mem")
    mem.insert(b"only-l1", M.TOMBSTONE)
    mem.insert(b"e", b"")
    oldmem = {b"zz": b"oldmem", b"om": b"1", b"kA0000003xxxxxxx": M.TOMBSTONE}
    keys = all_queries([sorted(t) for t in l0 + l1]) + [b"om", b"e"]
    with db.Reader(metas, ctx) as reader:
        assert reader.set.stat("tables") == 5
        for internal in (False, True):
            assert reader.get_many([mem, oldmem], keys, internal=internal) == db.get_many([mem, oldmem], metas, keys,
                                                                                         internal=internal)
        assert reader.get_many([], keys, internal=True) == sstable.get_many(metas, keys, ctx)
        assert reader.get_many([mem], [b"zz", b"q"]) == [b"mem", None] and reader.get_many([], []) == []
    with db.Reader([], ctx) as reader:
        assert reader.get_many([mem], [b"zz", b"q"]) == [b"mem", None]
