"""The reference's ``Db`` for many keys and many commands: the read side
(src/tokio/db.rs:144-189, src/sync/lsm_storage.rs:101) and the write side
(src/sync/lsm_storage.rs:59-78, 133-139).

``Db::get_internal`` asks the memtable (db.rs:158-165), then the old memtable
(db.rs:166-173), then every level's tables newest first (db.rs:178-185); the
first ``Some`` answers, and ``Db::get`` turns a ``Some`` of the one byte 0 --
what ``Db::delete`` inserts (db.rs:140) -- into ``None`` (db.rs:146-151).
``get_many`` is that loop: literally without a context, and as one
``lsmck_db_get_batch`` call with one -- the memtables become sorted runs, the
tables' files are uploaded once, and the values come back gathered in one
arena.

``LsmStorage::insert`` appends to the WAL, updates the memtable and flushes it
to a level-0 table when ``size_in_bytes() >= memtable_limit_bytes``
(lsm_storage.rs:65); ``delete`` inserts the value ``[0]`` and never flushes.
``write_many`` is that loop over a command stream: literally without a
context, and with one as a single ``lsmck_db_write_plan`` call -- the cuts and
every flushed memtable's entries -- whose entries go to one
``lsmck_sstable_encode_batch`` and whose last commands to one
``lsmck_wal_encode_batch``, all on the device.
"""
import time

import numpy as np

from . import _lib, sstable
from .sstable import TOMBSTONE_HIT

DELETED = b"\x00"  # the value Db::delete writes (db.rs:140)


def _items(memtable):
    """A memtable's (key, value) pairs in key order: a wal.MemTable or a dict."""
    data = memtable.data if hasattr(memtable, "data") else memtable
    return sorted((bytes(k), bytes(v)) for k, v in data.items())


def run_arrays(memtable):
    """A memtable as a run of lsmck_db_get_batch: (arena, arena, ents) -- keys
    and values back to back in one uint8 arena, WAL_CMD_DTYPE entries in key
    order."""
    items = _items(memtable)
    ents = np.zeros(len(items), dtype=_lib.WAL_CMD_DTYPE)
    klen = np.fromiter((len(k) for k, _ in items), dtype=np.uint64, count=len(items))
    vlen = np.fromiter((len(v) for _, v in items), dtype=np.uint64, count=len(items))
    start = np.cumsum(klen + vlen) - (klen + vlen)
    ents["type"], ents["klen"], ents["vlen"] = 1, klen, vlen
    ents["key_off"], ents["val_off"] = start, start + klen
    arena = np.frombuffer(b"".join(k + v for k, v in items), dtype=np.uint8)
    return arena, arena, ents


def get_many(memtables, levels, keys, ctx=None, internal=False):
    """Db::get for many keys.  ``memtables``: wal.MemTables or dicts, newest
    first (the memtable, then the old memtable); a delete is the value
    ``b"\\x00"``, as Db::delete writes it.  ``levels``: as in
    ``sstable.get_many``.  Without a context the literal loop runs: dict
    lookups, then ``sstable.table_get`` over the tables; with one, a single
    lsmck_db_get_batch call answers every key and the values are cut from the
    gathered arena.  Returns per key the value or None; with ``internal``
    get_internal's answer: TOMBSTONE_HIT where a tombstone answered.  The
    results are equal either way."""
    keys = [bytes(k) for k in keys]
    order = [m for level in levels for m in reversed(level)]
    datas = [open(m.data_path(), "rb").read() for m in order]
    idxs = [open(m.index_path(), "rb").read() for m in order]
    if ctx is None:
        dicts = [dict(_items(m)) for m in memtables]
        maps = [sstable.index_map(x) for x in idxs]
        out = []
        for k in keys:
            v = next((d[k] for d in dicts if k in d), None)
            if v is None:
                v = next((v for v in (sstable.table_get(d, None, k, m) for d, m in zip(datas, maps)) if v is not None),
                         None)
            out.append((TOMBSTONE_HIT if internal else None) if v == DELETED else v)
        return out
    spans = np.zeros(len(order), dtype=_lib.SSTABLE_SPAN_DTYPE)
    spans["data_len"], spans["index_len"] = [len(d) for d in datas], [len(x) for x in idxs]
    spans["data_off"] = np.cumsum(spans["data_len"]) - spans["data_len"]
    spans["index_off"] = np.cumsum(spans["index_len"]) - spans["index_len"]
    q = np.zeros(len(keys), dtype=_lib.GET_QUERY_DTYPE)
    klen = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
    q["klen"], q["key_off"] = klen, np.cumsum(klen) - klen
    res, off, vals = ctx.db_get_batch([run_arrays(m) for m in memtables], np.frombuffer(b"".join(datas), np.uint8),
                                      np.frombuffer(b"".join(idxs), np.uint8), spans,
                                      np.frombuffer(b"".join(keys), np.uint8), q)
    arena, off, out = vals.tobytes(), off.tolist(), []
    for i, (table, val_off) in enumerate(zip(res["table"].tolist(), res["val_off"].tolist())):
        if table == _lib.GET_NONE:
            out.append(None)
        elif val_off & _lib.GET_TOMBSTONE:
            out.append(TOMBSTONE_HIT if internal else None)
        else:
            out.append(arena[off[i]:off[i + 1]])
    return out


class Reader:
    """A reader that loads its tables once (SsTable::load,
    tokio/sstable.rs:32-55) and then serves gets until a compaction replaces
    them: ``levels``' files are read once and opened as one
    lsmck_tableset_open set on ``ctx`` -- the index pass and the tables' key
    fences stay on the device -- and ``get_many`` is one
    lsmck_tableset_get_batch call.  ``bloom_bits`` > 0 (4..64) also keeps a
    resident bloom filter per table at that many bits per key (the option
    "bloom_bits" is set around the open and restored).  ``close()`` frees the
    set."""

    def __init__(self, levels, ctx, bloom_bits=0):
        self.levels = [list(level) for level in levels]  # (apply_many's literal loop reads the files again)
        order = [m for level in self.levels for m in reversed(level)]
        datas = [open(m.data_path(), "rb").read() for m in order]
        idxs = [open(m.index_path(), "rb").read() for m in order]
        spans = np.zeros(len(order), dtype=_lib.SSTABLE_SPAN_DTYPE)
        spans["data_len"], spans["index_len"] = [len(d) for d in datas], [len(x) for x in idxs]
        spans["data_off"] = np.cumsum(spans["data_len"]) - spans["data_len"]
        spans["index_off"] = np.cumsum(spans["index_len"]) - spans["index_len"]
        before = ctx.get_stat("bloom_bits")
        ctx.set_option("bloom_bits", bloom_bits)
        try:
            self.set = ctx.tableset_open(np.frombuffer(b"".join(datas), np.uint8),
                                         np.frombuffer(b"".join(idxs), np.uint8), spans)
        finally:
            ctx.set_option("bloom_bits", before)

    def get_many(self, memtables, keys, internal=False):
        """``get_many(memtables, levels, keys, ctx, internal)`` over the opened tables: the same answers."""
        keys = [bytes(k) for k in keys]
        q = np.zeros(len(keys), dtype=_lib.GET_QUERY_DTYPE)
        klen = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
        q["klen"], q["key_off"] = klen, np.cumsum(klen) - klen
        res, off, vals = self.set.get_batch([run_arrays(m) for m in memtables], np.frombuffer(b"".join(keys), np.uint8), q)
        arena, off, out = vals.tobytes(), off.tolist(), []
        for i, (table, val_off) in enumerate(zip(res["table"].tolist(), res["val_off"].tolist())):
            if table == _lib.GET_NONE:
                out.append(None)
            elif val_off & _lib.GET_TOMBSTONE:
                out.append(TOMBSTONE_HIT if internal else None)
            else:
                out.append(arena[off[i]:off[i + 1]])
        return out

    def close(self):
        self.set.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _write_loop(base_path, commands, limit, stamps):
    """LsmStorage::insert / delete, command by command (lsm_storage.rs:59-78, 133-139)."""
    from . import wal
    mt, log, metas = wal.MemTable(), wal.CommandLog.new_in_memory(), []
    for c in commands:
        if isinstance(c, wal.Insert):
            log.insert(c.key, c.val)
            mt.insert(c.key, c.val)
            if mt.bytes >= limit:
                metas.append(sstable.from_memtable(base_path, mt, ctx=None, timestamp_ms=stamps(len(metas))))
                log = wal.CommandLog.new_in_memory()  # (wal.close() deletes the file, a new one is created)
                mt = wal.MemTable()
        else:
            log.remove(c.key)
            mt.insert(c.key, DELETED)
    return metas, mt, log.inner()


def _plan_results(ctx, dev, base_path, stamps, dk, dv, keys, vals, dents, nent, nflush, segs, log_cmds, log_ptr):
    """What write_many and apply_many make of a plan on the device: the flushed
    segments' tables (one lsmck_sstable_encode_batch), the memtable left, and
    the WAL image of ``log_cmds`` (at ``log_ptr`` on the device; one
    lsmck_wal_encode_batch) -- the writes behind the last flush."""
    from . import wal
    from .device import SstEncodeError
    first = segs["first_ent"].copy()  # the flushed tables' table_first
    metas = []
    if nflush:
        args = (dk.ptr, keys.nbytes, dv.ptr, vals.nbytes, dents.ptr, int(first[nflush]), first)
        try:  # the sizes: an index file holds its count at least, so no buffer at all is too small
            ctx.sstable_encode_batch_device(*args, None, 0, None, 0)
            raise AssertionError("an index file is never empty")
        except SstEncodeError as e:
            if e.needed is None:
                raise
            db, ib = e.needed
        data, index, dspans, sha = dev(db), dev(ib), dev(32 * nflush), dev(64 * nflush)
        got = ctx.sstable_encode_batch_device(*args, data.ptr, db, index.ptr, ib, dspans.ptr, sha.ptr,
                                              sha.ptr + 32 * nflush)
        assert got == (db, ib)
        hd, hx = memoryview(data.download(np.uint8, db)), memoryview(index.download(np.uint8, ib))
        spans = dspans.download(_lib.SSTABLE_SPAN_DTYPE, nflush)
        digests = sha.download(np.uint8, 64 * nflush).reshape(2, nflush, 32)
        for t in range(nflush):
            sp = spans[t]
            d0, i0 = int(sp["data_off"]), int(sp["index_off"])
            m = sstable.SsTableMetadata.new(base_path, 0, timestamp_ms=stamps(t))
            metas.append(sstable._write_table(m, hd[d0:d0 + int(sp["data_len"])], hx[i0:i0 + int(sp["index_len"])],
                                              digests[1][t], digests[0][t]))
    # the memtable left and its commands' log
    mt = wal.MemTable()
    e0 = int(first[nflush])
    ents = dents.download(_lib.WAL_CMD_DTYPE, nent - e0, 32 * e0)
    kb, vb = keys.tobytes(), vals.tobytes()
    for ko, kl, vo, vl in zip(ents["key_off"].tolist(), ents["klen"].tolist(), ents["val_off"].tolist(),
                              ents["vlen"].tolist()):
        mt.data[kb[ko:ko + kl]] = vb[vo:vo + vl]
    mt.bytes = int(segs["mem_bytes"][nflush])
    image = b""
    if len(log_cmds):
        size = ctx.lib.lsmck_wal_encoded_size(log_cmds.ctypes.data, len(log_cmds))
        dimg = dev(size)
        got = ctx.wal_encode_batch_device(dk.ptr, keys.nbytes, dv.ptr, vals.nbytes, log_ptr, len(log_cmds),
                                          dimg.ptr, size)
        assert got == size
        image = dimg.download(np.uint8, size).tobytes()
    return metas, mt, image


def write_many(base_path, commands, limit, ctx=None, timestamps_ms=None):
    """LsmStorage::insert / delete for a stream of ``wal.Insert`` /
    ``wal.Remove`` commands applied to a new, empty ``Db`` whose
    memtable_limit_bytes is ``limit``: every flush becomes a level-0 table
    under ``base_path`` (``timestamps_ms``: one per flush, in order).  Without
    a context the literal loop runs -- ``wal.MemTable.insert``, a
    ``CommandLog`` per memtable, ``sstable.from_memtable`` per flush; with one
    the commands go up once, lsmck_db_write_plan cuts them and orders every
    memtable, lsmck_sstable_encode_batch writes the flushed ones from its
    entries on the device and lsmck_wal_encode_batch frames the commands
    behind the last flush.  compact() behind a flush is the caller's
    (``sstable.merge_compact_many``).  Returns (the level-0 SsTableMetadata in
    flush order, the memtable left as a ``wal.MemTable`` -- a delete is the
    value ``b"\\x00"`` --, the WAL image).  The files and both other results
    are equal either way."""
    from . import wal
    commands = list(commands)
    t0 = int(time.time() * 1000)

    def stamps(i):
        return t0 + i if timestamps_ms is None else timestamps_ms[i]
    if ctx is None:
        return _write_loop(str(base_path), commands, limit, stamps)
    n = len(commands)
    cmds, _ = wal.encode_commands(commands)
    keys = np.frombuffer(b"".join(c.key for c in commands), dtype=np.uint8)
    vals = np.frombuffer(b"".join(c.val for c in commands if isinstance(c, wal.Insert)) + DELETED, dtype=np.uint8)
    tomb_off = len(vals) - 1  # the 0 byte a delete's entry points at
    bufs = []

    def dev(nbytes, src=None):
        b = ctx.alloc(max(nbytes, 1))
        bufs.append(b)
        if src is not None and src.nbytes:
            b.upload(src)
        return b
    try:
        dk, dv, dc = dev(keys.nbytes, keys), dev(vals.nbytes, vals), dev(cmds.nbytes, cmds)
        dents, dsegs = dev(32 * n), dev(24 * (n + 1))
        nent, nflush = ctx.db_write_plan_device(dk.ptr, keys.nbytes, dv.ptr, vals.nbytes, dc.ptr, n, limit, tomb_off,
                                                dents.ptr, n, None, dsegs.ptr, n + 1)
        segs = dsegs.download(_lib.WRITE_SEG_DTYPE, nflush + 1)
        c0 = int(segs["first_cmd"][nflush])
        return _plan_results(ctx, dev, str(base_path), stamps, dk, dv, keys, vals, dents, nent, nflush, segs,
                             cmds[c0:], dc.ptr + 32 * c0)
    finally:
        for b in bufs:
            b.free()


class Get:
    """Command::Get (src/command.rs): a read between the writes of ``apply_many``'s stream."""
    __slots__ = ("key",)

    def __init__(self, key):
        self.key = bytes(key)

    def __repr__(self):
        return f"Get({self.key!r})"

    def __eq__(self, other):
        return isinstance(other, Get) and other.key == self.key

    def __hash__(self):
        return hash(("Get", self.key))


def _apply_loop(base_path, commands, limit, stamps, levels, internal):
    """_write_loop with LsmStorage::get at every Get (lsm_storage.rs:99-125): the
    memtable, the stream's flushed tables newest first -- they lie behind the
    base's level-0 tables --, then the base's tables in search order."""
    from . import wal

    def opened(m):
        return open(m.data_path(), "rb").read(), sstable.index_map(open(m.index_path(), "rb").read())
    base = [opened(m) for level in levels for m in reversed(level)]
    mt, log, metas, flushed, out = wal.MemTable(), wal.CommandLog.new_in_memory(), [], [], []
    for c in commands:
        if isinstance(c, Get):
            v = mt.data.get(c.key)
            if v is None:
                v = next((v for v in (sstable.table_get(d, None, c.key, m) for d, m in flushed[::-1] + base)
                          if v is not None), None)
            out.append((TOMBSTONE_HIT if internal else None) if v == DELETED else v)
        elif isinstance(c, wal.Insert):
            log.insert(c.key, c.val)
            mt.insert(c.key, c.val)
            if mt.bytes >= limit:
                metas.append(sstable.from_memtable(base_path, mt, ctx=None, timestamp_ms=stamps(len(metas))))
                flushed.append(opened(metas[-1]))
                log = wal.CommandLog.new_in_memory()
                mt = wal.MemTable()
        else:
            log.remove(c.key)
            mt.insert(c.key, DELETED)
    return out, metas, mt, log.inner()


def apply_many(base_path, commands, limit, ctx=None, reader=None, timestamps_ms=None, internal=False):
    """LsmStorage::get / insert / delete for a stream of ``Get`` / ``wal.Insert``
    / ``wal.Remove`` commands in arrival order, every Get seeing every write
    before it, applied to a ``Db`` with an empty memtable whose tables -- the
    base -- are what ``reader`` (a ``Reader``; None: no table) holds and whose
    compact() is deferred, as in ``write_many``.  Returns (a response per Get
    in order: the value or None, with ``internal`` TOMBSTONE_HIT where a
    tombstone answered, as ``get_many`` gives; then ``write_many``'s three
    results: the level-0 SsTableMetadata in flush order, the memtable left, the
    WAL image -- Gets are not logged).  Without a context the literal loop
    runs, the base's files read from ``reader.levels``; with one the stream
    goes up once and a single lsmck_db_apply_plan call cuts it, orders every
    memtable and answers every Get a write of the stream answers -- those
    values are cut from the value arena --, the misses go to
    ``reader.set.get_batch`` in one call, and the encode and WAL steps are
    ``write_many``'s.  The results are equal either way, files included."""
    from . import wal
    commands = list(commands)
    t0 = int(time.time() * 1000)

    def stamps(i):
        return t0 + i if timestamps_ms is None else timestamps_ms[i]
    if ctx is None:
        return _apply_loop(str(base_path), commands, limit, stamps, reader.levels if reader is not None else [], internal)
    n = len(commands)
    is_get = np.fromiter((isinstance(c, Get) for c in commands), dtype=bool, count=n)
    cmds, _ = wal.encode_commands(commands)  # (a Get comes out as a Remove of its key)
    cmds["type"][is_get] = _lib.CMD_GET
    keys = np.frombuffer(b"".join(c.key for c in commands), dtype=np.uint8)
    vals = np.frombuffer(b"".join(c.val for c in commands if isinstance(c, wal.Insert)) + DELETED, dtype=np.uint8)
    tomb_off = len(vals) - 1
    bufs = []

    def dev(nbytes, src=None):
        b = ctx.alloc(max(nbytes, 1))
        bufs.append(b)
        if src is not None and src.nbytes:
            b.upload(src)
        return b
    try:
        dk, dv, dc = dev(keys.nbytes, keys), dev(vals.nbytes, vals), dev(cmds.nbytes, cmds)
        ng = int(is_get.sum())
        dents, dsegs, dgets, dmq, dmg = dev(32 * n), dev(24 * (n + 1)), dev(24 * ng), dev(16 * ng), dev(4 * ng)
        nent, nflush, nget, nmiss = ctx.db_apply_plan_device(
            dk.ptr, keys.nbytes, dv.ptr, vals.nbytes, dc.ptr, n, limit, tomb_off, dents.ptr, n, None, dsegs.ptr, n + 1,
            dgets.ptr, ng, dmq.ptr, dmg.ptr)
        assert nget == ng
        gets = dgets.download(_lib.APPLY_GET_DTYPE, nget)
        # the misses: the base's in one call
        out = [None] * nget
        if nmiss and reader is not None:
            miss_q, miss_get = dmq.download(_lib.GET_QUERY_DTYPE, nmiss), dmg.download(np.uint32, nmiss)
            res, off, got = reader.set.get_batch([], keys, miss_q)
            arena, off = got.tobytes(), off.tolist()
            for i, (g, table, val_off) in enumerate(zip(miss_get.tolist(), res["table"].tolist(), res["val_off"].tolist())):
                if table == _lib.GET_NONE:
                    continue
                out[g] = (TOMBSTONE_HIT if internal else None) if val_off & _lib.GET_TOMBSTONE else arena[off[i]:off[i + 1]]
        vb = vals.tobytes()
        for g, (source, val_off, vlen) in enumerate(zip(gets["source"].tolist(), gets["val_off"].tolist(),
                                                        gets["vlen"].tolist())):
            if source == _lib.GET_NONE:
                continue
            if val_off & _lib.GET_TOMBSTONE:
                out[g] = TOMBSTONE_HIT if internal else None
            else:
                out[g] = vb[val_off:val_off + vlen]
        segs = dsegs.download(_lib.WRITE_SEG_DTYPE, nflush + 1)
        c0 = int(segs["first_cmd"][nflush])
        log_cmds = np.ascontiguousarray(cmds[c0:][~is_get[c0:]])  # the writes behind the last flush
        dlog = dev(log_cmds.nbytes, log_cmds)
        return (out,) + _plan_results(ctx, dev, str(base_path), stamps, dk, dv, keys, vals, dents, nent, nflush, segs,
                                      log_cmds, dlog.ptr)
    finally:
        for b in bufs:
            b.free()


__all__ = ["get_many", "Reader", "run_arrays", "write_many", "apply_many", "Get", "TOMBSTONE_HIT", "DELETED"]
