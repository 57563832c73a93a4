"""The read side of the reference's ``Db`` (src/tokio/db.rs:144-189,
src/sync/lsm_storage.rs:101) for many keys.

``Db::get_internal`` asks the memtable (db.rs:158-165), then the old memtable
(db.rs:166-173), then every level's tables newest first (db.rs:178-185); the
first ``Some`` answers, and ``Db::get`` turns a ``Some`` of the one byte 0 --
what ``Db::delete`` inserts (db.rs:140) -- into ``None`` (db.rs:146-151).
``get_many`` is that loop: literally without a context, and as one
``lsmck_db_get_batch`` call with one -- the memtables become sorted runs, the
tables' files are uploaded once, and the values come back gathered in one
arena.
"""
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


__all__ = ["get_many", "run_arrays", "TOMBSTONE_HIT", "DELETED"]
