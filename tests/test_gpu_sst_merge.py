"""lsmck_sstable_decode_batch and lsmck_sstable_merge_batch on the GPU against
the cases module's expected values (merge_cases.py: the literal iterator and
the literal merge_compact loop, whose meaning tests/test_merge_cases.py proves
on the CPU), entry for entry through the arenas; the outputs between 0xAA
guards that must stay intact, as must everything past nent / nout.  The arenas
are allocated at exactly their size.  Then the chain decode, merge, encode
against table_bytes of the loop's output and hashlib, and sstable.merge_compact
with and without a context."""
import filecmp
import hashlib

import numpy as np
import pytest

import merge_cases as M
from lsm_storage_engine_amd import _lib, sstable
from lsm_storage_engine_amd.device import SstDecodeError, SstMergeError
from lsm_storage_engine_amd.sstable_metadata import SsTableMetadata

pytestmark = pytest.mark.gpu
AA = 0xAA
G = M.GUARD


class Dev:
    """Device buffers of one test: exact-size uploads, outputs filled with 0xAA between guards."""

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
        d = self.alloc(2 * G + nbytes)
        self.ctx.memset(d.ptr, AA, d.nbytes)
        return d

    def free(self):
        for d in self.bufs:
            d.free()


def inside(d, used, dtype):
    """The first `used` bytes between the guards as dtype, and whether every other byte is still 0xAA."""
    raw = d.download()
    ok = (raw[:G] == AA).all() and (raw[G + used:] == AA).all()
    return raw[G:G + used].view(dtype), bool(ok)


# --- decode ---------------------------------------------------------------------------------
def run_decode(ctx, b, with_index=True, cap=None, want_declined=0):
    pairs, first, cons = b.expected()
    nent = int(first[-1])
    cap = nent + 3 if cap is None else cap
    ntab = len(b.datas)
    d = Dev(ctx)
    try:
        dd, dx, ds = d.up(b.data), d.up(b.index), d.up(b.spans)
        de, dc = d.guarded(32 * cap), d.guarded(8 * ntab)
        ctx.sync()
        got, tf = ctx.sstable_decode_batch_device(dd.ptr, b.data.nbytes, dx.ptr if with_index else None, b.index.nbytes,
                                                  ds.ptr, ntab, de.ptr + G, cap, dc.ptr + G)
        declined = ctx.get_stat("sst_decode_declined")
        print("decode: nent", got, "expected", nent, "declined", declined, "expected", want_declined if with_index else 0)
        assert got == nent and tf.tolist() == first.tolist()
        assert declined == (want_declined if with_index else 0)
        ents, ok = inside(de, 32 * nent, _lib.WAL_CMD_DTYPE)
        assert ok
        c, ok = inside(dc, 8 * ntab, np.uint64)
        assert ok and c.tolist() == cons.tolist()
        assert (ents["type"] == 1).all() and (ents["reserved"] == 0).all()
        assert M.through_arena(b.data, ents) == [p for t in pairs for p in t]
        return ents.copy()
    finally:
        d.free()


def both_ways(ctx, b, want_declined=0):
    a = run_decode(ctx, b, True, want_declined=want_declined)
    p = run_decode(ctx, b, False)
    assert a.tobytes() == p.tobytes()
    return a


def images(tables):
    return [M.data_image(t) for t in tables], [M.index_image(t) for t in tables]


@pytest.mark.parametrize("front", range(16))
def test_decode_sizes_at_every_residue(ctx, front):
    """Tables of 0, 1, 99, 100, 101, 199, 200, 201 and 1,000 entries, the first
    at arena residue `front`, the last flush against the end of its allocation
    (the order rotates, so every size is the last one for some residue)."""
    sizes = M.DECODE_SIZES[front % 9:] + M.DECODE_SIZES[:front % 9]
    b = M.Batch(*images([M.table(m, m + front) for m in sizes]), front=front)
    both_ways(ctx, b)


def test_decode_every_cut_of_the_last_record(ctx):
    """101 and 201 entries with the last record cut by 1 byte .. all of it (1..7
    header bytes left, inside the key, inside the value, one byte short), every
    cut a table of one batch; the index is the one of the whole records."""
    datas, idxs = [], []
    for m in (1, 101, 201):
        t = M.table(m, 4)
        data, last = M.data_image(t), 8 + len(t[-1][0]) + len(t[-1][1])
        for cut in range(1, last + 1):
            datas.append(data[:-cut])
            idxs.append(M.index_image(t[:-1]))
    both_ways(ctx, M.Batch(datas, idxs, front=5))
    # the uncut table's index over a cut image: its last item names the cut record, so it is refused
    t = M.table(201, 4)
    b = M.Batch([M.data_image(t)[:-3], M.data_image(t)], [M.index_image(t)] * 2)
    both_ways(ctx, b, want_declined=1)


@pytest.mark.parametrize("ntab", [1, 63, 64, 65, 257])
def test_decode_table_counts(ctx, ntab):
    both_ways(ctx, M.Batch(*images([M.table((t * 37) % 130, t) for t in range(ntab)]), front=ntab % 16))


def test_decode_300k_entries_across_scan_blocks(ctx):
    """5,000 tables of 60 entries: the per-table scans cross their 4,096-item blocks."""
    tables = [M.table(60, t % 7) for t in range(7)]
    datas, idxs = images(tables)
    b = M.Batch([datas[t % 7] for t in range(5000)], [idxs[t % 7] for t in range(5000)], front=1)
    both_ways(ctx, b)


def test_decode_damaged_indexes(ctx):
    t = M.table(250, 3)
    data, good = M.data_image(t), M.index_image(t)
    damaged = M.damaged_indexes(t)
    for name, x in damaged:
        print("damaged index:", name)
        both_ways(ctx, M.Batch([data, data, data], [good, x, good], front=3), want_declined=1)
    # all of them in one batch, good ones between them
    idxs = [y for _, x in damaged for y in (x, good)]
    both_ways(ctx, M.Batch([data] * len(idxs), idxs), want_declined=len(damaged))
    # an empty index over records, an index over an empty table
    none = M.index_image([])
    both_ways(ctx, M.Batch([data, b"", b"abc"], [none, good, none]), want_declined=2)


def test_decode_indexes_with_keys_of_one_length(ctx):
    """The index's items a fixed step apart: proven by a thread per item
    (stat "sst_decode_uniform"), damaged ones refused, and an index whose key
    lengths only add up as equal ones would parsed serially and accepted."""
    sizes = [1, 99, 100, 101, 200, 201, 1000]
    b = M.Batch(*images([M.fixed_table(m, m) for m in sizes]), front=11)
    both_ways(ctx, b)
    run_decode(ctx, b, True)
    assert ctx.get_stat("sst_decode_uniform") == len(sizes)
    t = M.fixed_table(250, 2)
    data, good = M.data_image(t), M.index_image(t)
    damaged = M.damaged_indexes(t)
    idxs = [y for _, x in damaged for y in (x, good)]
    both_ways(ctx, M.Batch([data] * len(idxs), idxs, front=2), want_declined=len(damaged))
    odd = M.fixed_table(250, 1)
    odd[0], odd[100], odd[200] = (b"a00000", b""), (b"a100", b"x"), (b"a2000000", b"yy")  # 6 + 4 + 8 = 3 * 6
    b = M.Batch(*images([odd, t]))
    run_decode(ctx, b, True)
    assert ctx.get_stat("sst_decode_uniform") == 1


def test_decode_errors_write_nothing(ctx):
    t = M.table(120, 1)
    b = M.Batch(*images([t, t, t]))
    d = Dev(ctx)
    try:
        dd, dx = d.up(b.data), d.up(b.index)
        de, dc = d.guarded(32 * 400), d.guarded(8 * 3)
        dl = int(b.spans[1]["data_len"])
        for field, value, with_index in (("data_off", b.data.nbytes - dl + 1, True),  # one byte past the arena
                                         ("data_len", 1 << 32, True), ("data_off", 2 ** 64 - 4, False),
                                         ("index_len", b.index.nbytes, True)):
            spans = b.spans.copy()
            spans[1][field] = value
            ds = d.up(spans)
            with pytest.raises(SstDecodeError) as ei:
                ctx.sstable_decode_batch_device(dd.ptr, b.data.nbytes, dx.ptr if with_index else None, b.index.nbytes,
                                                ds.ptr, 3, de.ptr + G, 400, dc.ptr + G)
            assert ei.value.rc == _lib.EINVAL and ei.value.bad_index == 1, field
            assert inside(de, 0, np.uint8)[1] and inside(dc, 0, np.uint8)[1]
        ds = d.up(b.spans)
        with pytest.raises(SstDecodeError) as ei:
            ctx.sstable_decode_batch_device(dd.ptr, b.data.nbytes, dx.ptr, b.index.nbytes, ds.ptr, 3, de.ptr + G, 359,
                                            dc.ptr + G)
        assert ei.value.rc == _lib.ENOSPC and ei.value.needed == 360
        assert inside(de, 0, np.uint8)[1] and inside(dc, 0, np.uint8)[1]
    finally:
        d.free()


def test_decode_host_form(ctx):
    b = M.Batch(*images([M.table(m, m) for m in (0, 250, 1, 100)]), front=7)
    pairs, first, cons = b.expected()
    for index in (b.index, None):
        ents, tf, c = ctx.sstable_decode_batch(b.data, b.spans, index)
        assert tf.tolist() == first.tolist() and c.tolist() == cons.tolist()
        assert M.through_arena(b.data, ents) == [p for t in pairs for p in t]
    ents, tf, c = ctx.sstable_decode_batch(np.zeros(0, np.uint8), np.zeros(0, _lib.SSTABLE_SPAN_DTYPE))
    assert len(ents) == 0 and tf.tolist() == [0]


# --- merge ----------------------------------------------------------------------------------
MODES = {"stuck": "continue", "drop": "drop", "keep": "keep"}


def run_merge(ctx, b, tombstones, cap=None):
    want = b.expected(MODES[tombstones])
    n = len(b.ents)
    cap = n + 3 if cap is None else cap
    d = Dev(ctx)
    try:
        da, de = d.up(b.arena), d.up(b.ents)
        do, dsrc = d.guarded(32 * cap), d.guarded(4 * cap)
        ctx.sync()
        args = (da.ptr, b.arena.nbytes, da.ptr, b.arena.nbytes, de.ptr, n, b.tab_first, b.group_first, do.ptr + G, cap,
                dsrc.ptr + G)
        if not isinstance(want[0], list):  # the loop sticks: want is the tagged winner it holds
            with pytest.raises(SstMergeError) as ei:
                ctx.sstable_merge_batch_device(*args, tombstones=tombstones)
            print("merge: stuck at", ei.value.bad_index, "expected", want[2])
            assert ei.value.stuck and ei.value.rc == _lib.MERGE_STUCK and ei.value.bad_index == want[2]
            assert inside(do, 0, np.uint8)[1] and inside(dsrc, 0, np.uint8)[1]
            return None
        pairs, src, first = want
        nout, of = ctx.sstable_merge_batch_device(*args, tombstones=tombstones)
        print("merge:", tombstones, "nout", nout, "expected", len(pairs))
        assert nout == len(pairs) and of.tolist() == first.tolist()
        out, ok = inside(do, 32 * nout, _lib.WAL_CMD_DTYPE)
        assert ok
        s, ok = inside(dsrc, 4 * nout, np.uint32)
        assert ok and s.tolist() == src
        assert (out["type"] == 1).all() and (out["reserved"] == 0).all()
        assert M.through_arena(b.arena, out) == pairs
        return out.copy()
    finally:
        d.free()


def test_merge_groups_one_by_one(ctx):
    """Every group of merge_groups() as a batch of its own (k of 1, 2, 3, 4 and
    7, disjoint, interleaved, identical, an empty table, an empty group)."""
    for name, tables in M.merge_groups()[:11]:
        print("group:", name)
        run_merge(ctx, M.MergeBatch([tables]), "stuck")


def test_merge_one_key_against_a_table(ctx):
    """The one-key tables against tables of 0, 1, 2, 3 and 2^k +- 1 entries (below all of it,
    above all, equal to its first and its last; as the older and as the newer table), each
    position as a batch of its own groups."""
    groups = M.merge_groups()[11:]
    for name in ("below", "above", "first", "last"):
        run_merge(ctx, M.MergeBatch([tables for n, tables in groups if n.startswith("one " + name)]), "stuck")


def test_merge_all_groups_in_one_batch(ctx):
    """All of them as the groups of one batch -- the one-key tables against
    tables of 0, 1, 2, 3 and 2^k +- 1 entries among them -- in every mode."""
    b = M.MergeBatch([tables for _, tables in M.merge_groups()])
    a = run_merge(ctx, b, "stuck")
    assert a.tobytes() == run_merge(ctx, b, "drop").tobytes() == run_merge(ctx, b, "keep").tobytes()


@pytest.mark.parametrize("name,tables,key", M.tombstone_groups(), ids=[g[0] for g in M.tombstone_groups()])
def test_merge_tombstones(ctx, name, tables, key):
    b = M.MergeBatch([tables])
    for mode in MODES:
        run_merge(ctx, b, mode)


def test_merge_tombstones_across_groups(ctx):
    """Groups of 1 and 3 tables with an empty group among them; the first group that sticks is reported."""
    plain = [t for _, t in M.merge_groups()[3:6]]
    toms = M.tombstone_groups()
    b = M.MergeBatch([plain[0], [], toms[1][1], toms[7][1], plain[1], toms[0][1]])
    assert b.expected("continue")[0] == b"b"  # (the group of three, not the later "wins")
    for mode in MODES:
        run_merge(ctx, b, mode)


def test_merge_across_scan_blocks(ctx):
    """4 tables of 3,000 entries over 4,500 distinct keys of 16 bytes: the live flags' scan crosses its blocks."""
    rng = np.random.default_rng(11)
    keys = [b"key-%012d" % i for i in range(4500)]
    tabs = [[(keys[i], b"%d:%d" % (t, i)) for i in sorted(rng.choice(4500, size=3000, replace=False).tolist())]
            for t in range(4)]
    run_merge(ctx, M.MergeBatch([tabs, tabs[:2]]), "stuck")


def test_merge_validation(ctx):
    b = M.MergeBatch([[M._tab(M.POOL[:9], 0), M._tab(M.POOL[4:20], 1)], [M._tab(M.POOL[10:30], 2)]])
    n = len(b.ents)
    d = Dev(ctx)
    try:
        da = d.up(b.arena)
        do, dsrc = d.guarded(32 * n), d.guarded(4 * n)

        def call(ents, cap=n, tombstones="keep"):
            de = d.up(ents)
            return ctx.sstable_merge_batch_device(da.ptr, b.arena.nbytes, da.ptr, b.arena.nbytes, de.ptr, n, b.tab_first,
                                                  b.group_first, do.ptr + G, cap, dsrc.ptr + G, tombstones=tombstones)
        cases = []
        e = b.ents.copy()
        e[[12, 13]] = e[[13, 12]]  # an unsorted table
        cases.append((e, 13))
        e = b.ents.copy()
        e[30] = e[29]  # a repeated key inside a table
        cases.append((e, 30))
        e = b.ents.copy()
        e[3]["type"] = 2
        cases.append((e, 3))
        e = b.ents.copy()
        e[n - 1]["vlen"] += 1  # one byte past the arena
        cases.append((e, n - 1))
        e = b.ents.copy()
        e[5]["key_off"] = 2 ** 64 - 1
        e[20]["klen"] = 0xFFFFFFFF
        cases.append((e, 5))
        for ents, bad in cases:
            with pytest.raises(SstMergeError) as ei:
                call(ents)
            assert ei.value.rc == _lib.EINVAL and ei.value.bad_index == bad and not ei.value.stuck
            assert inside(do, 0, np.uint8)[1] and inside(dsrc, 0, np.uint8)[1]
        # LSMCK_ENOSPC at cap = nout - 1
        nout, _ = call(b.ents)
        ctx.memset(do.ptr, AA, do.nbytes)
        ctx.memset(dsrc.ptr, AA, dsrc.nbytes)
        with pytest.raises(SstMergeError) as ei:
            call(b.ents, cap=nout - 1)
        assert ei.value.rc == _lib.ENOSPC and ei.value.needed == nout
        assert inside(do, 0, np.uint8)[1] and inside(dsrc, 0, np.uint8)[1]
    finally:
        d.free()


def test_merge_host_form(ctx):
    b = M.MergeBatch([tables for _, tables in M.merge_groups()[:8]] + [M.tombstone_groups()[1][1]])
    pairs, src, first = b.expected("continue")
    out, s, of = ctx.sstable_merge_batch(b.arena, b.arena, b.ents, b.tab_first, b.group_first)
    assert s.tolist() == src and of.tolist() == first.tolist() and M.through_arena(b.arena, out) == pairs
    out, s, of = ctx.sstable_merge_batch(b.arena, b.arena, b.ents[:0], [0], [0])
    assert len(out) == 0 and of.tolist() == [0]
    # a memtable build's output is a valid table
    keys = np.frombuffer(b"bbaacc", dtype=np.uint8)
    cmds = np.zeros(3, dtype=_lib.WAL_CMD_DTYPE)
    cmds["key_off"], cmds["klen"], cmds["val_off"], cmds["vlen"], cmds["type"] = [0, 2, 4], 2, [0, 2, 4], 2, 1
    ents, _, _ = ctx.memtable_build(keys, keys, cmds)
    out, s, of = ctx.sstable_merge_batch(keys, keys, np.concatenate([ents, ents[1:]]), [0, 3, 5], [0, 2])
    assert M.through_arena(keys, out) == [(b"aa", b"aa"), (b"bb", b"bb"), (b"cc", b"cc")] and s.tolist() == [0, 3, 4]


# --- the chain and the files ------------------------------------------------------------------
def test_chain_decode_merge_encode(ctx):
    groups = [[M.table(250, 0), M.table(130, 2), M.table(300, 4)], [M.table(99, 1)], [], [M.table(101, 6), M.table(0, 0)]]
    tables = [t for g in groups for t in g]
    b = M.Batch(*images(tables), front=9)
    gf = np.zeros(len(groups) + 1, dtype=np.uint64)
    gf[1:] = np.cumsum([len(g) for g in groups])
    want = [M.merge_compact_loop(g, "keep") for g in groups]
    d = Dev(ctx)
    try:
        dd, dx, ds = d.up(b.data), d.up(b.index), d.up(b.spans)
        cap = b.data.nbytes // 8
        de, do = d.alloc(32 * cap), d.alloc(32 * cap)
        nent, tf = ctx.sstable_decode_batch_device(dd.ptr, b.data.nbytes, dx.ptr, b.index.nbytes, ds.ptr, len(tables),
                                                   de.ptr, cap)
        assert ctx.get_stat("sst_decode_declined") == 0
        nout, of = ctx.sstable_merge_batch_device(dd.ptr, b.data.nbytes, dd.ptr, b.data.nbytes, de.ptr, nent, tf, gf,
                                                  do.ptr, cap, tombstones="keep")
        assert of.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        files = [sstable.table_bytes(w) for w in want]
        ndb, nib = sum(len(f[0]) for f in files), sum(len(f[1]) for f in files)
        ng = len(groups)
        nd, nx, nsp, nsha = d.alloc(ndb), d.alloc(nib), d.alloc(32 * ng), d.alloc(64 * ng)
        got = ctx.sstable_encode_batch_device(dd.ptr, b.data.nbytes, dd.ptr, b.data.nbytes, do.ptr, nout, of, nd.ptr,
                                              ndb, nx.ptr, nib, nsp.ptr, nsha.ptr, nsha.ptr + 32 * ng)
        assert got == (ndb, nib)
        assert nd.download(np.uint8, ndb).tobytes() == b"".join(f[0] for f in files)
        assert nx.download(np.uint8, nib).tobytes() == b"".join(f[1] for f in files)
        sha = nsha.download(np.uint8, 64 * ng).reshape(2, ng, 32)
        for g, f in enumerate(files):
            assert sha[0][g].tobytes() == hashlib.sha256(f[0]).digest()
            assert sha[1][g].tobytes() == hashlib.sha256(f[1]).digest()
    finally:
        d.free()


def write_tables(base, level, tables, t0):
    return [sstable._write_table(SsTableMetadata.new(str(base), level, timestamp_ms=t0 + i), *sstable.table_bytes(t))
            for i, t in enumerate(tables)]


def same_table(a, b):
    return all(filecmp.cmp(getattr(a, p)(), getattr(b, p)(), shallow=False)
               for p in ("data_path", "index_path", "checksum_path"))


def test_merge_compact_files(ctx, tmp_path):
    tom = M.TOMBSTONE
    tables = [M.table(250, 0), [(b"kA0000003xxxxxxx", b"new"), (b"zz", tom)], M.table(120, 2) + [(b"zz", b"live")]]
    old = write_tables(tmp_path / "old", 0, tables, 1000)
    assert [list(sstable.read_table(m)) for m in old] == tables
    for mode in ("stuck", "drop", "keep"):
        host = sstable.merge_compact(tmp_path / ("host-" + mode), 1, old, None, mode, timestamp_ms=5)
        dev = sstable.merge_compact(tmp_path / ("dev-" + mode), 1, old, ctx, mode, timestamp_ms=5)
        assert same_table(host, dev) and host.level == dev.level == 1
        assert list(sstable.read_table(dev)) == M.merge_compact_loop(tables, "keep")  # (the tombstone is shadowed)
    stuck = write_tables(tmp_path / "stuck", 0, [tables[0], tables[2], tables[1]], 2000)
    for c in (None, ctx):
        with pytest.raises(sstable.MergeStuck) as ei:
            sstable.merge_compact(tmp_path / "never", 1, stuck, c)
        assert ei.value.key == b"zz"
    for mode in ("drop", "keep"):
        host = sstable.merge_compact(tmp_path / ("host2-" + mode), 2, stuck, None, mode, timestamp_ms=6)
        dev = sstable.merge_compact(tmp_path / ("dev2-" + mode), 2, stuck, ctx, mode, timestamp_ms=6)
        assert same_table(host, dev)
        assert list(sstable.read_table(dev)) == M.merge_compact_loop([tables[0], tables[2], tables[1]], mode)


def test_merge_compact_many(ctx, tmp_path):
    jobs_tables = [[M.table(101, 0), M.table(60, 2)], [M.table(5, 1)], [M.table(300, 4), M.table(300, 4), M.table(7, 6)]]
    jobs, t0 = [], 100
    for j, tabs in enumerate(jobs_tables):
        jobs.append((1 + j % 2, write_tables(tmp_path / "old", 0, tabs, t0), 9000 + j))
        t0 += 10
    new = sstable.merge_compact_many(tmp_path / "new", jobs, ctx, "keep")
    assert len(new) == 3
    for (level, old, ts), m, tabs in zip(jobs, new, jobs_tables):
        host = sstable.merge_compact(tmp_path / "host", level, old, None, "keep", timestamp_ms=ts)
        assert same_table(host, m) and m.level == level
        assert list(sstable.read_table(m)) == M.merge_compact_loop(tabs, "keep")
