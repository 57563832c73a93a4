"""lsmck_db_get_batch on the GPU against the cases module's expected values
(dbget_cases.py: dict lookups over the runs, get_cases' table loop, b"".join
for the gather -- their meaning is proven on the CPU by
tests/test_dbget_cases.py), bit-exact.  Every arena is a device allocation of
exactly its size; res, out_off and out lie between 0xAA guards that must stay
intact, and after a refused call all three are still 0xAA.  Then the host
form, the chain log image -> device memtable -> run 0 over flushed tables, and
db.get_many with and without a context."""
import numpy as np
import pytest

import dbget_cases as D
import get_cases as G
import merge_cases as M
from lsm_storage_engine_amd import _lib, db, sstable, wal
from lsm_storage_engine_amd.device import DbGetError

pytestmark = pytest.mark.gpu
AA = 0xAA
GUARD = M.GUARD
TOMB = M.TOMBSTONE


class Dev:
    """Device buffers of one test: exact-size uploads, the outputs filled with 0xAA between guards."""

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

    def guarded(self, nbytes, residue=0):
        d = self.alloc(2 * GUARD + 16 + nbytes)
        self.ctx.memset(d.ptr, AA, d.nbytes)
        d.at = GUARD + residue  # the output's first byte
        return d

    def free(self):
        for d in self.bufs:
            d.free()


def inside(d, nbytes):
    raw = d.download()
    ok = (raw[:d.at] == AA).all() and (raw[d.at + nbytes:] == AA).all()
    return raw[d.at:d.at + nbytes].copy(), bool(ok)


def device_get(ctx, b, values=True, residue=0, out_cap=None, ents=None, spans=None, q=None, shared=False):
    """The device form over exact-size uploads: (res, out_off, out, every byte
    outside them still 0xAA).  ents: the runs' entries, doctored; shared: the
    runs' arenas and entries in ONE device buffer; out_cap: None = exactly the
    expected bytes."""
    spans = b.spans if spans is None else spans
    q = b.q if q is None else q
    n = len(q)
    want_total = len(b.expected_out) if out_cap is None else out_cap
    d = Dev(ctx)
    try:
        desc = np.zeros(len(b.runs), dtype=_lib.GET_RUN_DTYPE)
        if shared:
            pieces, at = [], 0
            for r, run in enumerate(b.runs):
                e = run.ents if ents is None else ents[r]
                row = []
                for a in (run.keys, run.vals, e.view(np.uint8)):
                    at += (-at) % 8
                    row.append(at)
                    pieces.append((at, a))
                    at += a.nbytes
                desc[r] = (row[0], run.keys.nbytes, row[1], run.vals.nbytes, row[2], len(e))
            buf = np.zeros(at, dtype=np.uint8)
            for o, a in pieces:
                buf[o:o + a.nbytes] = a.view(np.uint8)
            base = d.up(buf).ptr
            for f in ("keys", "vals", "ents"):
                desc[f] += base
        else:
            for r, run in enumerate(b.runs):
                e = run.ents if ents is None else ents[r]
                dk = d.up(run.keys)
                dv = dk if run.vals is run.keys else d.up(run.vals)
                desc[r] = (dk.ptr, run.keys.nbytes, dv.ptr, run.vals.nbytes, d.up(e).ptr, len(e))
        dd, dx, ds, dqk, dq = d.up(b.data), d.up(b.index), d.up(spans), d.up(b.qkeys), d.up(q)
        dres, doff, dout = d.guarded(16 * n), d.guarded(8 * (n + 1)), d.guarded(want_total, residue)
        ctx.sync()
        args = (desc, dd.ptr, b.data.nbytes, dx.ptr, b.index.nbytes, ds.ptr, len(spans), dqk.ptr, b.qkeys.nbytes, dq.ptr,
                n, dres.ptr + dres.at)
        try:
            if values:
                total = ctx.db_get_batch_device(*args, dout.ptr + dout.at, want_total, doff.ptr + doff.at)
            else:
                total = ctx.db_get_batch_device(*args)
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


def check(ctx, b, want=None, **kw):
    want = b.expected() if want is None else want
    b.expected_out = want[2]
    res, off, out, ok = device_get(ctx, b, **kw)
    bad = np.nonzero(res != want[0])[0]
    print("db get: queries", len(b.q), "runs", len(b.runs), "tables", len(b.spans), "answered bytes", len(want[2]),
          "mismatches", len(bad))
    assert ok, "guards"
    assert len(bad) == 0, [(int(i), b.keys[i], res[i], want[0][i]) for i in bad[:5]]
    assert np.array_equal(off, want[1]) and np.array_equal(out, want[2])
    return res, off, out


def all_queries(tables, light=True):
    seen, out = set(), []
    for t in tables:
        for k in G.queries_for(t, light):
            if k not in seen:
                seen.add(k)
                out.append(k)
    return out


@pytest.mark.parametrize("res", range(16))
def test_run_sizes_at_every_residue(ctx, res):
    """Runs of 0, 1, 2, 63, 64 and 65 entries in rotating search order -- key
    lengths 0..17, 24 and 25, keys equal in their first 8 bytes, proper
    prefixes -- the key arena at residue `res`, the value arena at another,
    every third residue both in one arena; the last key and value flush with
    the allocations' ends.  Every present key, and absent keys below, above,
    between, prefixes, a key plus one byte, the empty key."""
    sizes = D.RUN_SIZES[res % 6:] + D.RUN_SIZES[:res % 6]
    pairs = [D.run_pairs(m, res + j) for j, m in enumerate(sizes)]
    runs = [D.Run(p, res, (res * 7 + j) % 16, one=(res + j) % 3 == 0) for j, p in enumerate(pairs)]
    for p, run in zip(pairs, runs):  # each run alone: every key of it is found, and nothing else
        got, _, _ = check(ctx, D.DbGetBatch([run], [], all_queries([p], light=False), qfront=res % 5))
        assert int((got["table"] == 0).sum()) == len(p)
    b = D.DbGetBatch(runs, [], all_queries(pairs, light=False), qfront=res % 5)  # and all six in search order
    check(ctx, b)


def test_no_runs_equals_the_point_read(ctx):
    """nrun == 0 over get_cases' sized, tie and quirk tables: byte-identical to lsmck_sstable_get_batch's expected results."""
    sized = [G.images(t) for _, t in G.sized_tables()]
    batches = [G.GetBatch(sized, all_queries([t for _, t in G.sized_tables()]), front=7, qfront=3)]
    tabs = [(e, s) for _, e, s in G.tie_tables()]
    batches.append(G.GetBatch([G.images(e, s) for e, s in tabs], all_queries([e for e, _ in tabs], light=False)))
    e, T = G.QUIRK_ENTRIES, G.quirk_tables()
    keys = [k for k, _ in e] + [b"", b"q", b"q00100x", b"q0010", b"q00150xx\x00", b"zzz"]
    batches += [G.GetBatch([tab, T["plain"]], keys, front=7) for name, tab in T.items()]
    for g in batches:
        b = D.DbGetBatch([], g.tables, g.keys, front=int(g.spans["data_off"][0]) if len(g.spans) else 0,
                         qfront=int(g.q["key_off"][0]) if len(g.q) else 0)
        assert np.array_equal(b.data, g.data) and np.array_equal(b.qkeys, g.qkeys)
        got, _, _ = check(ctx, b)
        assert got.tobytes() == g.expected().tobytes()
        res, off, out, ok = device_get(ctx, b, values=False)  # out_off == NULL: out stays untouched
        assert ok and res.tobytes() == got.tobytes() and len(off) == 0 and len(out) == 0


def test_degenerate_shapes(ctx):
    """ntab == 0; nrun == ntab == 0; n == 0."""
    runs, tabs, keys = D.precedence()
    R = [D.Run(runs[0], 3, 5), D.Run(runs[1], 1, 2, one=True)]
    got, _, _ = check(ctx, D.DbGetBatch(R, [], keys, qfront=2))
    assert set(got["table"].tolist()) == {0, 1, D.NONE_SOURCE}
    got, off, out = check(ctx, D.DbGetBatch([], [], keys))
    assert (got["table"] == D.NONE_SOURCE).all() and (got["val_off"] == 0).all() and (off == 0).all() and len(out) == 0
    got, off, out = check(ctx, D.DbGetBatch(R, [G.images(t) for t in tabs], []))
    assert len(got) == 0 and off.tolist() == [0]
    got, off, out = check(ctx, D.DbGetBatch([], [], []))
    assert len(got) == 0 and off.tolist() == [0]
    b = D.DbGetBatch([D.Run([]), D.Run([])], [G.images([])], keys)  # empty sources
    got, _, _ = check(ctx, b)
    assert (got["table"] == D.NONE_SOURCE).all()


def test_precedence(ctx):
    """The hand-worked cases of tests/test_dbget_cases.py, and the two runs in one device buffer."""
    runs, tabs, keys = D.precedence()
    b = D.DbGetBatch([D.Run(runs[0], 3, 5), D.Run(runs[1], 1, 2, one=True)], [G.images(t) for t in tabs], keys,
                     front=3, qfront=1)
    for shared in (False, True):
        got, off, out = check(ctx, b, shared=shared)
        assert got["table"].tolist() == [0, 0, 0, 0, D.NONE_SOURCE, 0, 1, 1, 2, 2, D.NONE_SOURCE, D.NONE_SOURCE]
        assert (got["val_off"] >> np.uint64(63)).tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0]
        assert out.tobytes() == b"from-run0againfrom-run0run1-onlytable-only"
        assert b.values(got) == [b"from-run0", TOMB, b"again", b"", None, b"from-run0", b"run1-only", TOMB,
                                 b"table-only", TOMB, None, None]


def test_overlapping_index_spans(ctx):
    """Thirty tables that read one index image behind a run: more items than the
    index arena's bytes suggest, so the item scratch grows and every pass runs again."""
    ents = [(bytes([65 + i]), b"v%d" % i) for i in range(40)]
    run = [(b"B", b"from-the-run"), (b"Bx", b""), (b"zz", TOMB)]
    b = D.DbGetBatch([D.Run(run, 1, 2)], [G.images(ents, 1)], all_queries([ents, run], light=False))
    want = b.expected()
    b.expected_out = want[2]
    res, off, out, ok = device_get(ctx, b, spans=np.repeat(b.spans, 30))
    assert ok and np.array_equal(res, want[0]) and np.array_equal(off, want[1]) and np.array_equal(out, want[2])


def gather_batch(res):
    """Values of every length of D.GATHER_LENGTHS in run 0's value arena (at
    residue res) and again in table 0's data file (the arena at residue res);
    queries: runs of zero-length answers at the start, in the middle and at
    the end, every value once from each source, one of them twice."""
    lens = D.GATHER_LENGTHS
    run = [(b"g%02d" % i, D.value_of(n, i + res)) for i, n in enumerate(lens)] + [(b"gdead", TOMB)]
    tab = [(b"t%02d" % i, D.value_of(n, 40 + i + res)) for i, n in enumerate(lens)] + [(b"tdead", TOMB)]
    zero = [b"miss0", b"g00", b"gdead", b"tdead", b"t00"]
    keys = zero + [k for pair in zip([k for k, _ in run[:-1]], [k for k, _ in tab[:-1]]) for k in pair]
    keys = keys[:20] + zero[::-1] + keys[20:] + [b"g03"] + zero
    return D.DbGetBatch([D.Run(sorted(run), res % 4, res)], [G.images(sorted(tab))], keys, front=res, qfront=res % 3)


@pytest.mark.parametrize("res", range(16))
def test_gather_at_every_residue(ctx, res):
    """Value lengths 0 .. 65537 (inside one 32 KiB tile, across a tile's
    boundary, over three tiles) from a run's vals and from data, the sources
    and `out` at residue `res`; out_cap exact."""
    b = gather_batch(res)
    want = b.expected()
    got, off, out = check(ctx, b, want, residue=res)
    assert int(off[-1]) == 2 * sum(D.GATHER_LENGTHS) + D.GATHER_LENGTHS[3]
    assert (np.diff(off.astype(np.int64))[:5] == 0).all() and (np.diff(off.astype(np.int64))[-5:] == 0).all()


def test_gather_small_totals_and_no_space(ctx):
    """A total under 16 bytes, a total of 0, out_cap = total - 1 (ENOSPC names the total, nothing is written), out_off == NULL."""
    run = [(b"a", b"12345"), (b"b", b""), (b"c", TOMB), (b"d", b"6789")]
    for res in (0, 9, 15):
        b = D.DbGetBatch([D.Run(run, 1, res)], [], [b"x", b"a", b"b", b"c", b"d", b"a", b"x"])
        _, off, out = check(ctx, b, residue=res)
        assert out.tobytes() == b"12345678912345" and off.tolist() == [0, 0, 5, 5, 5, 9, 14, 14]
        b = D.DbGetBatch([D.Run(run, 1, res)], [], [b"x", b"b", b"c", b"c"])
        _, off, out = check(ctx, b, residue=res)
        assert len(out) == 0 and off.tolist() == [0] * 5
    b = gather_batch(5)
    want = b.expected()
    b.expected_out = want[2]
    with pytest.raises(DbGetError) as ei:
        device_get(ctx, b, residue=5, out_cap=len(want[2]) - 1)
    assert (ei.value.rc, ei.value.needed, ei.value.bad_run_entry) == (_lib.ENOSPC, len(want[2]), None)
    with pytest.raises(DbGetError) as ei:
        device_get(ctx, b, out_cap=0)
    assert (ei.value.rc, ei.value.needed) == (_lib.ENOSPC, len(want[2]))
    res, off, out, ok = device_get(ctx, b, values=False)
    assert ok and np.array_equal(res, want[0]) and len(off) == 0 and len(out) == 0


def refused(ctx, b, run=None, table=None, query=None, **kw):
    b.expected_out = np.zeros(64, dtype=np.uint8)
    with pytest.raises(DbGetError) as ei:
        device_get(ctx, b, **kw)
    e = ei.value
    print("refused: bad_run_entry", e.bad_run_entry, "bad_table", e.bad_table, "bad_query", e.bad_query)
    assert (e.bad_run_entry, e.bad_table, e.bad_query, e.rc) == (run, table, query, _lib.EINVAL)


def test_refusals(ctx):
    """Each names the first offender, counted across the runs, and leaves res, out_off and out untouched."""
    p0, p1 = D.run_pairs(10, 0), D.run_pairs(12, 2)
    e = G.QUIRK_ENTRIES
    data, good = G.images(e)
    b = D.DbGetBatch([D.Run(p0, 2, 3), D.Run(p1, 1, 0, one=True)], [(data, good)] * 2, [e[3][0], p0[4][0], b""])
    fresh = lambda: [r.ents.copy() for r in b.runs]  # noqa: E731
    ents = fresh()
    ents[1][4] = ents[1][3]
    refused(ctx, b, run=10 + 4, ents=ents)  # equal adjacent keys
    ents = fresh()
    ents[0][[6, 7]] = ents[0][[7, 6]]
    refused(ctx, b, run=7, ents=ents)  # a decreasing pair
    ents = fresh()
    ents[1]["vlen"][11] += 1  # (the last value of the shared arena: one byte past it)
    refused(ctx, b, run=10 + 11, ents=ents)
    ents = fresh()
    ents[0]["key_off"][2] = 2 ** 64 - 2
    refused(ctx, b, run=2, ents=ents)
    ents = fresh()
    ents[0]["val_off"][5], ents[0]["vlen"][5] = b.runs[0].vals.nbytes, 1
    refused(ctx, b, run=5, ents=ents)
    ents = fresh()
    ents[1]["type"][0] = 2  # type 2 in a run
    ents[1]["klen"][5] = 0xFFFFFFFF
    refused(ctx, b, run=10, ents=ents)
    ents = fresh()
    assert int(ents[0]["klen"][0]) == 0
    ents[0]["key_off"][0] = 2 ** 64 - 1  # (an empty key's offset is not looked at)
    b.expected_out = b.expected()[2]
    res, _, _, ok = device_get(ctx, b, ents=ents)
    assert ok and np.array_equal(res, b.expected()[0])
    # a bad run entry, a refused index and a bad query in one batch: run, then table, then query
    ents = fresh()
    ents[1]["type"][2] = 0
    bad_x = dict(G.refused_indexes())["count-1"]
    bx = D.DbGetBatch(b.runs, [(data, good), (data, bad_x)], b.keys)
    q = bx.q.copy()
    q["reserved"][2] = 1
    refused(ctx, bx, run=12, ents=ents, q=q)
    refused(ctx, bx, table=1, q=q)
    refused(ctx, b, query=2, q=q)
    refused(ctx, b, run=12, ents=ents, q=q, values=False)


@pytest.fixture(scope="module")
def seeded():
    runs, tabs, keys = D.seeded()
    b = D.DbGetBatch([D.Run(runs[0], 5, 9), D.Run(runs[1], 2, 0, one=True)], [G.images(t) for t in tabs], keys,
                     front=11, qfront=2)
    return b, b.expected(fast=True, entries=tabs)


def test_seeded_batch(ctx, seeded):
    """2 runs of about 1,000 entries, 8 tables of about 300, 4,096 queries; the stage timer and the stats."""
    b, want = seeded
    got, _, _ = check(ctx, b, want, residue=7)
    srcs = set(got["table"].tolist())
    assert {0, 1, 2, D.NONE_SOURCE} <= srcs
    ctx.set_option("sst_encode_time", 1)
    try:
        check(ctx, b, want)
        stats = {k: ctx.get_stat(k) for k in ("db_get_runs_ns", "db_get_index_ns", "db_get_run_probe_ns", "db_get_probe_ns",
                                              "db_get_resolve_ns", "db_get_gather_ns", "db_get_probed", "db_get_walked",
                                              "db_get_run_hits")}
        print("stats", stats)
        assert all(v > 0 for v in stats.values())
        assert stats["db_get_run_hits"] == int((got["table"] < 2).sum())
        # a query a run answered costs the table probe no lookup
        assert stats["db_get_walked"] <= stats["db_get_probed"] <= (len(b.q) - stats["db_get_run_hits"]) * len(b.spans)
    finally:
        ctx.set_option("sst_encode_time", 0)


def test_host_form_equals_device_form(ctx, seeded):
    b, want = seeded
    runs = [r.arrays() for r in b.runs]
    for pinned in (False, True):
        res, off, out = ctx.db_get_batch(runs, b.data, b.index, b.spans, b.qkeys, b.q, pinned=pinned)
        assert np.array_equal(res, want[0]) and np.array_equal(off, want[1]) and np.array_equal(out, want[2])
    res, off, out = ctx.db_get_batch(runs, b.data, b.index, b.spans, b.qkeys, b.q, values=False)
    assert np.array_equal(res, want[0]) and off is None and out is None
    res, off, out = ctx.db_get_batch(runs, b.data, b.index, b.spans, b.qkeys, b.q[:0])  # n == 0
    assert len(res) == 0 and off.tolist() == [0] and len(out) == 0
    res, off, out = ctx.db_get_batch([], b.data[:0], b.index[:0], b.spans[:0], b.qkeys, b.q[:5])  # no source
    assert (res["table"] == D.NONE_SOURCE).all() and off.tolist() == [0] * 6
    g = gather_batch(3)  # (more bytes than the first guess: the call is made again with the size it names)
    res, off, out = ctx.db_get_batch([r.arrays() for r in g.runs], g.data, g.index, g.spans, g.qkeys, np.tile(g.q, 4))
    w = g.expected()
    assert np.array_equal(res, np.tile(w[0], 4)) and out.tobytes() == w[2].tobytes() * 4
    ents = b.runs[1].ents.copy()
    ents["type"][7] = 2
    with pytest.raises(DbGetError) as ei:
        ctx.db_get_batch([runs[0], (runs[1][0], runs[1][1], ents)], b.data, b.index, b.spans, b.qkeys, b.q)
    assert (ei.value.bad_run_entry, ei.value.bad_table, ei.value.bad_query) == (len(b.runs[0].ents) + 7, None, None)


def log_image(ops):
    log = wal.CommandLog.new_in_memory()
    for k, v in ops:
        log.log(wal.Remove(k) if v is None else wal.Insert(k, v))
    return log.inner()


def test_chain_device_memtable_over_flushed_tables(ctx, tmp_path):
    """A log image -> wal.device_memtable, used as run 0 where it lies, over
    tables written by flush_many; equal to db.get_many without a context,
    whose memtable is MemTable.from_log's dict."""
    old = [dict(M.table(150, 0)), dict(M.table(101, 2) + [(b"zz", b"old"), (b"gone", b"still-here")])]
    metas = sstable.flush_many(str(tmp_path), 0, [sorted(t.items()) for t in old], ctx, timestamps_ms=[1000, 2000])
    ops = [(b"zz", b"newest"), (b"kA0000003xxxxxxx", b"over"), (b"tmp", b"x"), (b"tmp", None), (b"gone", TOMB),
           (b"e", b""), (b"zz", b"newest-2")] + [(b"w%03d" % i, b"log-%d" % i * (i % 7)) for i in range(200)]
    image = log_image(ops)
    mem = wal.MemTable.from_log(wal.CommandLog.new_in_memory(image))
    keys = all_queries([sorted(t.items()) for t in old] + [sorted(mem.data.items())]) + [b"tmp"]
    want = db.get_many([mem], [metas], keys, internal=True)
    order = metas[::-1]
    datas = [open(m.data_path(), "rb").read() for m in order]
    idxs = [open(m.index_path(), "rb").read() for m in order]
    t = G.GetBatch(list(zip(datas, idxs)), keys, qfront=1)
    dm = wal.device_memtable(image, ctx)
    d = Dev(ctx)
    try:
        assert dm.nent == len(mem.data)
        dd, dx, ds, dqk, dq = d.up(t.data), d.up(t.index), d.up(t.spans), d.up(t.qkeys), d.up(t.q)
        n = len(keys)
        total = sum(len(v) for v in want if v not in (None, sstable.TOMBSTONE_HIT))
        dres, doff, dout = d.guarded(16 * n), d.guarded(8 * (n + 1)), d.guarded(total, 3)
        got = ctx.db_get_batch_device([dm], dd.ptr, t.data.nbytes, dx.ptr, t.index.nbytes, ds.ptr, 2, dqk.ptr, t.qkeys.nbytes,
                                      dq.ptr, n, dres.ptr + dres.at, dout.ptr + dout.at, total, doff.ptr + doff.at)
        assert got == total
        (res, ok1), (off, ok2), (out, ok3) = inside(dres, 16 * n), inside(doff, 8 * (n + 1)), inside(dout, total)
        assert ok1 and ok2 and ok3
        res, off, out = res.view(_lib.GET_RESULT_DTYPE), off.view(np.uint64).tolist(), out.tobytes()
        vals = [None if int(r["table"]) == _lib.GET_NONE else sstable.TOMBSTONE_HIT if int(r["val_off"]) >> 63
                else out[off[i]:off[i + 1]] for i, r in enumerate(res)]
        assert vals == want
        at = {k: i for i, k in enumerate(keys)}
        assert vals[at[b"zz"]] == b"newest-2" and int(res[at[b"zz"]]["table"]) == 0
        assert vals[at[b"gone"]] is sstable.TOMBSTONE_HIT and vals[at[b"tmp"]] is None and vals[at[b"e"]] == b""
        assert int(res[at[b"e"]]["table"]) == 0 and int(res[at[sorted(old[0])[5]]]["table"]) == 2
    finally:
        d.free()
        dm.free()


def test_get_many_files(ctx, tmp_path):
    """db.get_many with and without a context, on files: memtables newest first in front of sstable.get_many's levels."""
    l0 = [M.table(120, 0), M.table(101, 2) + [(b"zz", b"old")], [(b"kA0000003xxxxxxx", b"newest"), (b"zz", TOMB)]]
    l1 = [M.table(250, 0), [(b"only-l1", b"deep"), (b"zz", b"l1")]]
    metas = [[sstable._write_table(sstable.SsTableMetadata.new(str(tmp_path), lvl, timestamp_ms=1000 * lvl + i),
                                   *sstable.table_bytes(sorted(t))) for i, t in enumerate(level)]
             for lvl, level in enumerate((l0, [], l1))]
    mem = wal.MemTable()
    mem.insert(b"zz", b"mem")
    mem.insert(b"only-l1", TOMB)  # Db::delete
    mem.insert(b"e", b"")
    oldmem = {b"zz": b"oldmem", b"om": b"1", b"kA0000003xxxxxxx": TOMB}
    keys = all_queries([sorted(t) for t in l0 + l1]) + [b"om", b"e"]
    for internal in (False, True):
        host = db.get_many([mem, oldmem], metas, keys, internal=internal)
        dev = db.get_many([mem, oldmem], metas, keys, ctx, internal=internal)
        assert host == dev
    tables = sstable.get_many(metas, keys, ctx)
    dicts = [mem.data, oldmem]
    lit = [next((m[k] for m in dicts if k in m), t) for k, t in zip(keys, tables)]
    assert dev == [sstable.TOMBSTONE_HIT if v == TOMB else v for v in lit]
    at = {k: i for i, k in enumerate(keys)}
    assert dev[at[b"zz"]] == b"mem" and dev[at[b"only-l1"]] is sstable.TOMBSTONE_HIT and dev[at[b"om"]] == b"1"
    assert dev[at[b"kA0000003xxxxxxx"]] is sstable.TOMBSTONE_HIT and dev[at[b"e"]] == b""
    assert db.get_many([], metas, keys, ctx, internal=True) == tables
    assert db.get_many([mem], [], [b"zz", b"q"], ctx) == [b"mem", None] and db.get_many([], [], [], ctx) == []
