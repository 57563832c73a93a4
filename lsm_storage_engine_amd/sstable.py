"""Writing SSTables -- the host-side mirror of ``SsTable::from_memtable``
(src/tokio/sstable.rs:84-129, src/sync/sstable.rs:135-141,241-253).

A table is five files named by ``SsTableMetadata``: the data file
(``[u32 klen][u32 vlen][key][val]`` per entry in key order, datafile.rs:27-35),
the index file (bincode of the BTreeMap that maps every INDEX_STEP-th key to
its record's position, sstable_index.rs:42-46), the checksum JSON
(checksums.rs:64-80: ``index_checksum`` first, the file opened without
truncate), an empty bloom filter file (bloom filters are out of scope here, as
for ``tree.synthesize_tree``) and the metadata JSON.

``from_memtable`` writes one table; ``flush_many`` writes many from one GPU
call (``lsmck_sstable_encode_batch``: the data and index images of every table
and their SHA-256 digests).  Without a context the bytes are built here and
hashed by the scalar path (``Checksums.write_checksums``); the files are the
same either way.

Reading them back: ``read_table`` (the iterator), ``merge_compact`` (the
compaction) and the point read -- ``table_get``, SsTable::get literally, and
``get_many``, Db::get's table loop for many keys, one
``lsmck_sstable_get_batch`` with a context or the literal loop without one.
"""
import ctypes as C
import os
import struct
import time

import numpy as np

from . import _lib
from .checksums import Checksums
from .sstable_metadata import SsTableMetadata

INDEX_STEP = 100  # src/tokio/sstable.rs:17


def _entries(memtable):
    """(key, value) pairs in the memtable's BTreeMap order: a wal.MemTable, a
    dict, or an iterable of pairs."""
    items = memtable.data.items() if hasattr(memtable, "data") else \
        memtable.items() if hasattr(memtable, "items") else memtable
    return sorted((bytes(k), bytes(v)) for k, v in items)


def table_bytes(entries):
    """One table's data and index file contents from its sorted entries."""
    data, index, pos = bytearray(), [], 0
    for i, (k, v) in enumerate(entries):
        if i % INDEX_STEP == 0:
            index.append((k, pos))
        data += struct.pack("<II", len(k), len(v)) + k + v
        pos += 8 + len(k) + len(v)
    idx = bytearray(struct.pack("<Q", len(index)))
    for k, p in index:
        idx += struct.pack("<Q", len(k)) + k + struct.pack("<Q", p)
    return bytes(data), bytes(idx)


def batch_arrays(tables):
    """The arenas, entries (WAL_CMD_DTYPE, type 1) and table_first of
    lsmck_sstable_encode_batch for a list of tables' sorted entries: keys back
    to back in one arena, values in another."""
    flat = [e for t in tables for e in t]
    n = len(flat)
    ents = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    klen = np.fromiter((len(k) for k, _ in flat), dtype=np.uint64, count=n)
    vlen = np.fromiter((len(v) for _, v in flat), dtype=np.uint64, count=n)
    ents["klen"], ents["vlen"], ents["type"] = klen, vlen, 1
    ents["key_off"], ents["val_off"] = np.cumsum(klen) - klen, np.cumsum(vlen) - vlen
    keys = np.frombuffer(b"".join(k for k, _ in flat), dtype=np.uint8)
    vals = np.frombuffer(b"".join(v for _, v in flat), dtype=np.uint8)
    first = np.zeros(len(tables) + 1, dtype=np.uint64)
    first[1:] = np.cumsum([len(t) for t in tables])
    return keys, vals, ents, first


def _b64(digest):
    raw = bytes(digest)
    out = C.create_string_buffer(45)
    _lib.load().lsmck_base64_encode(raw, len(raw), out)
    return out.value.decode()


def _write_no_truncate(path, payload):
    fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)  # .write(true).create(true): no truncate, as the reference
    try:
        os.write(fd, payload)
    finally:
        os.close(fd)


def _write_checksum_json(path, index_sha, data_sha):
    """checksums.rs:64-80 from digests already computed: serde_json's compact
    form, index_checksum first, what lsmck_checksums_write leaves."""
    s = '{"index_checksum":"%s","data_checksum":"%s"}' % (_b64(index_sha), _b64(data_sha))
    _write_no_truncate(path, s.encode())


def _write_table(m, data, index, index_sha=None, data_sha=None):
    os.makedirs(os.path.dirname(m.data_path()), exist_ok=True)
    with open(m.data_path(), "wb") as f:
        f.write(data)
    with open(m.index_path(), "wb") as f:
        f.write(index)
    if index_sha is None:
        Checksums.write_checksums(m)  # the scalar path: both files read back and hashed on this thread
    else:
        _write_checksum_json(m.checksum_path(), index_sha, data_sha)
    open(m.bloom_filter_path(), "wb").close()
    m.write_to_file()
    return m


def flush_many(base_path, level, memtables, ctx, timestamps_ms=None):
    """Write one table per memtable under ``<base_path>/level-<level>``.  With
    a context every table's data and index image and both digests come from
    one lsmck_sstable_encode_batch call; with ``ctx=None`` they are built here
    and hashed one file at a time.  Returns the tables' SsTableMetadata."""
    tables = [_entries(mt) for mt in memtables]
    if timestamps_ms is None:
        t0 = int(time.time() * 1000)
        timestamps_ms = [t0 + i for i in range(len(tables))]
    metas = [SsTableMetadata.new(str(base_path), level, timestamp_ms=ts) for ts in timestamps_ms]
    assert len(metas) == len(tables)
    if ctx is None:
        return [_write_table(m, *table_bytes(t)) for m, t in zip(metas, tables)]
    if not tables:
        return []
    keys, vals, ents, first = batch_arrays(tables)
    data, index, spans, dsha, isha = ctx.sstable_encode_batch(keys, vals, ents, first)
    for t, m in enumerate(metas):
        s = spans[t]
        d0, i0 = int(s["data_off"]), int(s["index_off"])
        _write_table(m, memoryview(data)[d0:d0 + int(s["data_len"])], memoryview(index)[i0:i0 + int(s["index_len"])],
                     isha[t], dsha[t])
    return metas


def from_memtable(base_path, memtable, ctx=None, timestamp_ms=None):
    """SsTable::from_memtable: the memtable as a level-0 table.  Returns its SsTableMetadata."""
    ts = None if timestamp_ms is None else [timestamp_ms]
    return flush_many(base_path, 0, [memtable], ctx, ts)[0]


def flush_log_image(base_path, image, ctx, timestamp_ms=None):
    """A log image as a level-0 table, the whole chain on the device: replay,
    commands, memtable build (wal.device_memtable), then
    lsmck_sstable_encode_batch over the live entries with keys = vals = the
    image.  Only the data file, the index file and the two digests come back;
    no record or entry visits the host.  The files equal
    ``from_memtable(base_path, MemTable.from_log(CommandLog.new_in_memory(image)))``'s.
    Returns the table's SsTableMetadata."""
    from . import wal
    from .device import SstEncodeError
    d = wal.device_memtable(image, ctx)
    bufs = []
    try:
        first = [0, d.nent]
        args = (d.image.ptr, d.image_bytes, d.image.ptr, d.image_bytes, d.ents.ptr, d.nent, first)
        try:  # the sizes: the index file holds its count at least, so no buffer at all is too small
            ctx.sstable_encode_batch_device(*args, None, 0, None, 0)
            raise AssertionError("an index file is never empty")
        except SstEncodeError as e:
            if e.needed is None:
                raise
            db, ib = e.needed
        bufs = [ctx.alloc(max(db, 1)), ctx.alloc(ib), ctx.alloc(64)]
        data, index, sha = bufs
        got = ctx.sstable_encode_batch_device(*args, data.ptr, db, index.ptr, ib, None, sha.ptr, sha.ptr + 32)
        assert got == (db, ib)
        digests = sha.download(np.uint8, 64)
        m = SsTableMetadata.new(str(base_path), 0, timestamp_ms=timestamp_ms)
        return _write_table(m, data.download(np.uint8, db).data, index.download(np.uint8, ib).data, digests[32:],
                            digests[:32])
    finally:
        d.free()
        for b in bufs:
            b.free()


class MergeStuck(RuntimeError):
    """merge_compact met a tombstone (value ``[0]``) that wins its key: the
    reference's loop does ``continue`` there without advancing anything
    (src/sync/sstable.rs:193-195) and never terminates.  ``key`` is that key."""

    def __init__(self, key):
        self.key = bytes(key)
        super().__init__(f"merge_compact: the tombstone of key {self.key!r} wins; the reference's loop never "
                         f"terminates there (tombstones='drop' or 'keep' chooses a meaning)")


def iter_records(image):
    """The reference's iterator over a data file image (sync/sstable.rs:77-90,
    datafile.rs:60-83): (key, value) pairs from pos 0; UnexpectedEof anywhere
    -- the header, the key or the value cut -- ends the table cleanly."""
    image = bytes(image)
    pos = 0
    while len(image) - pos >= 8:
        klen, vlen = struct.unpack_from("<II", image, pos)
        if len(image) - pos - 8 < klen + vlen:
            return
        yield image[pos + 8:pos + 8 + klen], image[pos + 8 + klen:pos + 8 + klen + vlen]
        pos += (8 + klen + vlen) & 0xFFFFFFFF  # (u32, datafile.rs:81; a record that fits a file under 4 GiB cannot wrap)


def read_table(meta):
    """The (key, value) pairs the reference's iterator yields from the table's data file."""
    with open(meta.data_path(), "rb") as f:
        return iter_records(f.read())


def merge_loop(tables, tombstones="stuck"):
    """SsTable::merge_compact's loop (sync/sstable.rs:157-208), literally, over
    tables given as iterables of (key, value) in the reference's vector order
    (oldest first).  A tombstone winner raises MergeStuck ("stuck": the
    reference never terminates), is advanced past ("drop") or written
    ("keep").  Returns the pairs written, in order."""
    if tombstones not in ("stuck", "drop", "keep"):
        raise ValueError(tombstones)
    iterators = [iter(t) for t in tables]
    values = [next(it, None) for it in iterators]
    out = []
    while True:
        current = None
        for i in range(len(iterators)):
            kv = values[i]
            if kv is None:
                continue
            if current is None:
                current = i
            else:
                curr = current
                if kv[0] <= values[curr][0]:
                    current = i
                if values[curr][0] == kv[0]:
                    values[curr] = next(iterators[curr], None)
        if current is None:
            return out
        kv = values[current]
        if kv[1] == b"\x00":
            if tombstones == "stuck":
                raise MergeStuck(kv[0])
            if tombstones == "drop":
                values[current] = next(iterators[current], None)
                continue
        out.append(kv)
        values[current] = next(iterators[current], None)


def merge_compact_many(base_path, jobs, ctx, tombstones="stuck"):
    """Many compactions in one pass over the device: ``jobs`` is a list of
    (level, tables) or (level, tables, timestamp_ms), ``tables`` the
    SsTableMetadata of one merge in the reference's order (oldest first).  The
    old tables' data and index files are uploaded once; decode
    (lsmck_sstable_decode_batch, the index files as the proven hint), merge
    (lsmck_sstable_merge_batch, one group per job) and encode
    (lsmck_sstable_encode_batch) run on the device in one context, and only the
    new data files, index files and digests come back.  Removing the old
    tables stays with the caller.  Returns the new tables' SsTableMetadata."""
    from .device import SstEncodeError, SstMergeError
    jobs = [tuple(j) if len(j) == 3 else (j[0], j[1], None) for j in jobs]
    if not jobs:
        return []
    t0 = int(time.time() * 1000)
    metas = [SsTableMetadata.new(str(base_path), level, timestamp_ms=t0 + i if ts is None else ts)
             for i, (level, _, ts) in enumerate(jobs)]
    old = [m for _, tables, _ in jobs for m in tables]
    datas = [open(m.data_path(), "rb").read() for m in old]
    idxs = [open(m.index_path(), "rb").read() for m in old]
    spans = np.zeros(len(old), dtype=_lib.SSTABLE_SPAN_DTYPE)
    spans["data_len"], spans["index_len"] = [len(d) for d in datas], [len(x) for x in idxs]
    spans["data_off"] = np.cumsum(spans["data_len"]) - spans["data_len"]
    spans["index_off"] = np.cumsum(spans["index_len"]) - spans["index_len"]
    group_first = np.zeros(len(jobs) + 1, dtype=np.uint64)
    group_first[1:] = np.cumsum([len(tables) for _, tables, _ in jobs])
    arena, iarena = b"".join(datas), b"".join(idxs)
    db, ib, ntab = len(arena), len(iarena), len(old)
    bufs = []

    def alloc(nbytes):
        bufs.append(ctx.alloc(max(nbytes, 1)))
        return bufs[-1]
    try:
        d_data, d_index, d_spans = alloc(db), alloc(ib), alloc(32 * ntab)
        if db:
            d_data.upload(np.frombuffer(arena, np.uint8))
        if ib:
            d_index.upload(np.frombuffer(iarena, np.uint8))
        if ntab:
            d_spans.upload(spans)
        cap = db // 8  # (a record is 8 bytes or more, and the spans do not overlap)
        d_ents, d_out = alloc(32 * cap), alloc(32 * cap)
        nent, tab_first = ctx.sstable_decode_batch_device(d_data.ptr, db, d_index.ptr if ib else None, ib, d_spans.ptr,
                                                          ntab, d_ents.ptr, cap)
        try:
            nout, out_first = ctx.sstable_merge_batch_device(d_data.ptr, db, d_data.ptr, db, d_ents.ptr, nent, tab_first,
                                                             group_first, d_out.ptr, cap, tombstones=tombstones)
        except SstMergeError as e:
            if not e.stuck:
                raise
            c = d_ents.download(_lib.WAL_CMD_DTYPE, 1, 32 * e.bad_index)[0]
            raise MergeStuck(arena[int(c["key_off"]):int(c["key_off"]) + int(c["klen"])]) from e
        args = (d_data.ptr, db, d_data.ptr, db, d_out.ptr, nout, out_first)
        # The encode's size query (as in flush_log_image): with no buffers at all it runs its
        # size passes, writes nothing and reports LSMCK_ENOSPC with both sizes -- an index file
        # holds its count at least, so this call cannot succeed.
        try:
            ctx.sstable_encode_batch_device(*args, None, 0, None, 0)
            raise AssertionError("an index file is never empty")
        except SstEncodeError as e:
            if e.needed is None:
                raise
            ndb, nib = e.needed
        ng = len(jobs)
        n_data, n_index, n_spans, n_sha = alloc(ndb), alloc(nib), alloc(32 * ng), alloc(64 * ng)
        got = ctx.sstable_encode_batch_device(*args, n_data.ptr, ndb, n_index.ptr, nib, n_spans.ptr, n_sha.ptr,
                                              n_sha.ptr + 32 * ng)
        assert got == (ndb, nib)
        data, index = n_data.download(np.uint8, ndb), n_index.download(np.uint8, nib)
        nspans = n_spans.download(_lib.SSTABLE_SPAN_DTYPE, ng)
        sha = n_sha.download(np.uint8, 64 * ng).reshape(2, ng, 32)
    finally:
        for b in bufs:
            b.free()
    for g, m in enumerate(metas):
        sp = nspans[g]
        d0, i0 = int(sp["data_off"]), int(sp["index_off"])
        _write_table(m, memoryview(data)[d0:d0 + int(sp["data_len"])], memoryview(index)[i0:i0 + int(sp["index_len"])],
                     sha[1][g], sha[0][g])
    return metas


def merge_compact(base_path, level, tables, ctx=None, tombstones="stuck", timestamp_ms=None):
    """SsTable::merge_compact (src/sync/sstable.rs:151-224, tokio/sstable.rs:135-207):
    the tables (SsTableMetadata, in the reference's vector order: oldest first,
    the newest wins a key) merged into one table of ``level``.  With a context
    the files are uploaded once and decode, merge and encode run on the device
    (merge_compact_many); without one the literal loop runs here (merge_loop).
    The files are equal either way.  ``tombstones``: "stuck" raises MergeStuck
    where the reference's loop never terminates, "drop" leaves the key out,
    "keep" writes the tombstone.  Removing the old tables stays with the
    caller.  Returns the new table's SsTableMetadata."""
    if tombstones not in ("stuck", "drop", "keep"):
        raise ValueError(tombstones)
    if ctx is not None:
        return merge_compact_many(base_path, [(level, tables, timestamp_ms)], ctx, tombstones)[0]
    entries = merge_loop([read_table(m) for m in tables], tombstones)
    m = SsTableMetadata.new(str(base_path), level, timestamp_ms=timestamp_ms)
    return _write_table(m, *table_bytes(entries))


class _TombstoneHit:
    """get_many's result for a key whose first answer is a tombstone."""

    def __repr__(self):
        return "TOMBSTONE_HIT"


TOMBSTONE_HIT = _TombstoneHit()


def _read_record(image, pos):
    """datafile.rs:60-83: ((key, value), record length) or None on UnexpectedEof."""
    if pos > len(image) or len(image) - pos < 8:
        return None
    klen, vlen = struct.unpack_from("<II", image, pos)
    if len(image) - pos - 8 < klen + vlen:
        return None
    return (image[pos + 8:pos + 8 + klen], image[pos + 8 + klen:pos + 8 + klen + vlen]), 8 + klen + vlen


def index_map(index):
    """The index file's BTreeMap<Vec<u8>, u64> (sstable_index.rs:20-25) as
    (keys, positions) in key order.  Raises ValueError for an image that does
    not parse to exactly its length or whose keys do not strictly increase:
    the reference panics at load or never writes such a file, and
    lsmck_sstable_get_batch refuses it."""
    index = bytes(index)
    if len(index) < 8:
        raise ValueError("index: no count")
    (count,), at, keys, pos = struct.unpack_from("<Q", index, 0), 8, [], []
    for _ in range(count):
        if len(index) - at < 16:
            raise ValueError("index: an item is cut")
        klen = struct.unpack_from("<Q", index, at)[0]
        if klen > len(index) - at - 16:
            raise ValueError("index: an item is cut")
        key = index[at + 8:at + 8 + klen]
        if keys and not keys[-1] < key:
            raise ValueError("index: keys do not strictly increase")
        keys.append(key)
        pos.append(struct.unpack_from("<Q", index, at + 8 + klen)[0])
        at += 16 + klen
    if at != len(index):
        raise ValueError("index: trailing bytes")
    return keys, pos


def table_get(data, index, key, _map=None):
    """SsTable::get (src/sync/sstable.rs:97-113), literally, over a table's
    data and index file images: the value, or None.  An exact index hit
    returns the record at the item's position whatever its key is;
    otherwise the records from the last item below the key are scanned, the
    first one always read, until the position of the first item above it
    (datafile.rs:85-103).  The bloom filter is not read (a filter built from
    the table's own keys never changes a result)."""
    import bisect
    data, key = bytes(data), bytes(key)
    keys, pos = index_map(index) if _map is None else _map
    i = bisect.bisect_left(keys, key)
    if i < len(keys) and keys[i] == key:
        r = _read_record(data, pos[i])
        return None if r is None else r[0][1]
    p = pos[i - 1] if i > 0 else 0
    end = pos[i] if i < len(keys) else len(data)
    while True:
        r = _read_record(data, p)
        if r is None:
            return None
        if r[0][0] == key:
            return r[0][1]
        p += r[1]
        if p >= end:
            return None


def get_many(levels, keys, ctx=None):
    """Db::get_internal's table loop (src/tokio/db.rs:178-185) for many keys:
    ``levels`` is a list of lists of SsTableMetadata in the reference's vector
    order; every level is asked newest first (reversed), level 0 before level
    1 and so on, and the first table whose get is Some answers.  With a
    context the files are uploaded once and one lsmck_sstable_get_batch
    answers every key; without one table_get runs in a loop.  Returns per key
    the value, None (no table holds it) or TOMBSTONE_HIT (the first answer is
    the tombstone ``[0]``: Db::get's other kind of "not found", db.rs:146-151).
    The results are equal either way.  The memtables' step of Db::get stays
    with the caller."""
    keys = [bytes(k) for k in keys]
    order = [m for level in levels for m in reversed(level)]
    datas = [open(m.data_path(), "rb").read() for m in order]
    idxs = [open(m.index_path(), "rb").read() for m in order]
    if ctx is None:
        maps = [index_map(x) for x in idxs]
        out = []
        for k in keys:
            v = next((v for v in (table_get(d, None, k, m) for d, m in zip(datas, maps)) if v is not None), None)
            out.append(TOMBSTONE_HIT if v == b"\x00" else v)
        return out
    spans = np.zeros(len(order), dtype=_lib.SSTABLE_SPAN_DTYPE)
    spans["data_len"], spans["index_len"] = [len(d) for d in datas], [len(x) for x in idxs]
    spans["data_off"] = np.cumsum(spans["data_len"]) - spans["data_len"]
    spans["index_off"] = np.cumsum(spans["index_len"]) - spans["index_len"]
    arena = b"".join(datas)
    q = np.zeros(len(keys), dtype=_lib.GET_QUERY_DTYPE)
    klen = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
    q["klen"], q["key_off"] = klen, np.cumsum(klen) - klen
    res = ctx.sstable_get_batch(np.frombuffer(arena, np.uint8), np.frombuffer(b"".join(idxs), np.uint8), spans,
                                np.frombuffer(b"".join(keys), np.uint8), q)
    out = []
    for r in res:
        off = int(r["val_off"])
        if int(r["table"]) == _lib.GET_NONE:
            out.append(None)
        elif off & _lib.GET_TOMBSTONE:
            out.append(TOMBSTONE_HIT)
        else:
            out.append(arena[off:off + int(r["vlen"])])
    return out


__all__ = ["from_memtable", "flush_many", "flush_log_image", "table_bytes", "batch_arrays", "INDEX_STEP",
           "iter_records", "read_table", "merge_loop", "merge_compact", "merge_compact_many", "MergeStuck", "index_map", "table_get",
           "get_many", "TOMBSTONE_HIT"]
