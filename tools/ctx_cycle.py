#!/usr/bin/env python3
"""Device memory across a context's life: does a destroyed context give back
every buffer it grew?

One cycle creates a context, turns every "*_time" option on, takes each path
that grows a context buffer, compares every result with the oracle or the
package's CPU path, and closes the context:
  * a descriptor CRC batch and a SHA-256 batch from host memory (4,096 records
    of 0..5,000 bytes: the staging slots, the order scratch), the same CRC
    batch from device memory, a fixed 4 KiB batch of 1,024 records;
  * a ~4 MiB log of 40,000 Insert / Remove records replayed from device memory
    (defaults; "wal_seg_bytes" 262144: the emit's checkpoint arrays;
    "wal_seg_walk" 0: the candidate-doubling walk's arrays; the compact record
    layout; "wal_gpu_walk" 0: the pinned host copy and descriptor staging) and
    from host memory (defaults: the upload; "wal_upload_min" 0: the host walk);
  * wal_encode_batch, sstable_encode_batch and memtable_build in host form on
    those 40,000 commands;
  * checksums_verify_many on four small tables written by the package's writer.
Three cycles run.  After each, torch.cuda.synchronize() and the device's free
memory (torch.cuda.mem_get_info).  Cycle 1 absorbs the runtime's one-time
allocations; the figure is free memory after cycle 2 less free memory after
cycle 3.  Prints one JSON line.

Measured on an MI355X: 0 bytes on the commit before the buffers became owning
objects (every buffer freed by hand in lsmck_ctx_destroy), 0 bytes on the one
that made them so (profiles/r10/refactor/README.md).  tests/test_gpu_ctx_cycle.py
allows the parent's drop plus 2 MiB: the cycle's larger buffers (the log image, the
arenas, the record arrays, the staging slots) are each above that, so one of
them leaking fails the test.  Buffers smaller than the margin are not covered
by this tool: they are covered by the sanitizer test of the buffer type
(tests/test_growbuf_model.py: every block freed exactly once) and by review.

  python3 tools/ctx_cycle.py [--cycles 3]
"""
import argparse
import gc
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: the torch wheel's HIP runtime)
from lsm_storage_engine_amd import _lib, sstable, wal  # noqa: E402
from lsm_storage_engine_amd.device import Context, decode_rec16  # noqa: E402
from oracle import oracle as O  # noqa: E402

NREC = 40000


class Inputs:
    """Everything a cycle reads, with the expected results, built once."""

    def __init__(self, tmp):
        rng = np.random.default_rng(0)
        # smoke()'s descriptor batch
        n = 4096
        ln = rng.integers(0, 5000, n).astype(np.uint32)
        ln[:8] = [0, 1, 2, 3, 4, 127, 128, 129]
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(ln[:-1])
        off += 3
        self.off, self.ln = off, ln
        self.data = O.gen_stream(0x5EED0003, 0, int(off[-1]) + int(ln[-1]) + 8)
        self.crc = O.crc32_batch(self.data, off, ln)
        self.sha = O.sha256_batch(self.data, off, ln, threads=4)
        self.fixed_n = 1024
        self.fixed_crc = O.crc32_fixed(O.gen_stream(0x5EED0002, 0, self.fixed_n * 4096), 4096, 4096, self.fixed_n)
        # the log: 40,000 records, about 4 MiB, every 7th a Remove, keys that come back
        vlen = rng.integers(40, 150, NREC)
        blob = bytes(O.gen_stream(0x5EED0005, 0, 1 << 16))
        self.records = []
        for i in range(NREC):
            key = b"key%05d" % (i * 7919 % 30000)
            self.records.append(wal.Remove(key) if i % 7 == 6 else wal.Insert(key, blob[i:i + int(vlen[i])]))
        self.image = b"".join(O.wal_insert(r.key, r.val) if isinstance(r, wal.Insert) else O.wal_remove(r.key)
                              for r in self.records)
        st, recs, _ = O.wal_replay(self.image)
        assert st == 0 and len(recs) == NREC
        self.rec_off = [r.rec_off for r in recs]
        self.cmds, _ = wal.encode_commands(self.records)
        self.keys = np.frombuffer(b"".join(r.key for r in self.records), dtype=np.uint8)
        self.vals = np.frombuffer(b"".join(r.val for r in self.records if isinstance(r, wal.Insert)), dtype=np.uint8)
        # the memtable and four tables of it, on the CPU
        mt = wal.MemTable.from_log(wal.CommandLog.new_in_memory(self.image))
        self.entries, self.mem_bytes = sorted(mt.data.items()), mt.size_in_bytes()
        q = (len(self.entries) + 3) // 4
        self.tables = [self.entries[i:i + q] for i in range(0, len(self.entries), q)]
        self.table_files = [sstable.table_bytes(t) for t in self.tables]
        metas = sstable.flush_many(tmp, 0, [dict(t[:200]) for t in self.tables], None, [1000 + i for i in range(4)])
        self.triples = [(m.data_path(), m.index_path(), m.checksum_path()) for m in metas]


def replay(ctx, I, want_compact=False, **kw):
    recs, st, _ = ctx.wal_replay_verify(kw.pop("image"), compact=want_compact, **kw)
    if want_compact:
        recs = decode_rec16(recs)
    assert st == 0 and [int(x) for x in recs["rec_off"]] == I.rec_off, "WAL replay mismatch"


def cycle(I):
    ctx = Context(0)
    try:
        for k in ("wal_encode_time", "sst_encode_time", "mem_build_time"):
            ctx.set_option(k, 1)
        # host batches through the staging slots, the same batch on the device, fixed 4 KiB records
        assert np.array_equal(ctx.crc32(I.data, I.off, I.ln), I.crc), "crc32 host batch mismatch"
        assert np.array_equal(ctx.sha256(I.data, I.off, I.ln), I.sha), "sha256 host batch mismatch"
        n = len(I.ln)
        bufs = [ctx.alloc(x) for x in (len(I.data), 8 * n, 4 * n, 4 * n)]
        dd, doff, dlen, dout = bufs
        for b, a in ((dd, np.frombuffer(I.data, np.uint8)), (doff, I.off), (dlen, I.ln)):
            b.upload(a)
        ctx.crc32_device(dd.ptr, doff.ptr, dlen.ptr, n, dout.ptr)
        ctx.sync()
        assert np.array_equal(dout.download(np.uint32, n), I.crc), "crc32 device batch mismatch"
        dfix, dfo = ctx.alloc(I.fixed_n * 4096), ctx.alloc(4 * I.fixed_n)
        bufs += [dfix, dfo]
        ctx.gen_stream(dfix.ptr, 0x5EED0002, 0, I.fixed_n * 4096)
        ctx.crc32_fixed_device(dfix.ptr, 4096, 4096, I.fixed_n, dfo.ptr)
        ctx.sync()
        assert np.array_equal(dfo.download(np.uint32, I.fixed_n), I.fixed_crc), "crc32 fixed batch mismatch"
        # the log from device memory: every walk, both record layouts
        nb = len(I.image)
        dw = ctx.alloc(nb)
        bufs.append(dw)
        dw.upload(np.frombuffer(I.image, np.uint8))
        replay(ctx, I, image=nb, device_ptr=dw.ptr)
        for key, value, default in (("wal_seg_bytes", 262144, 0), ("wal_seg_walk", 0, 1), ("wal_gpu_walk", 0, 1)):
            ctx.set_option(key, value)
            replay(ctx, I, image=nb, device_ptr=dw.ptr)
            ctx.set_option(key, default)
        replay(ctx, I, want_compact=True, image=nb, device_ptr=dw.ptr)
        # ... and from host memory: uploaded, then walked on the host
        replay(ctx, I, image=I.image)
        ctx.set_option("wal_upload_min", 0)
        replay(ctx, I, image=I.image)
        ctx.set_option("wal_upload_min", 1 << 20)
        # the three builders, host form
        img, rec_off = ctx.wal_encode_batch(I.keys, I.vals, I.cmds)
        assert img.tobytes() == I.image and rec_off.tolist() == I.rec_off, "wal_encode_batch mismatch"
        keys, vals, ents, first = sstable.batch_arrays(I.tables)
        data, index, spans, dsha, isha = ctx.sstable_encode_batch(keys, vals, ents, first)
        assert data.tobytes() == b"".join(d for d, _ in I.table_files), "sstable_encode_batch data mismatch"
        assert index.tobytes() == b"".join(x for _, x in I.table_files), "sstable_encode_batch index mismatch"
        for t, (d, x) in enumerate(I.table_files):
            assert dsha[t].tobytes() == hashlib.sha256(d).digest() and isha[t].tobytes() == hashlib.sha256(x).digest(), \
                "sstable_encode_batch digest mismatch"
        ments, _, mem_bytes = ctx.memtable_build(I.keys, I.vals, I.cmds)
        kb, vb = I.keys.tobytes(), I.vals.tobytes()
        got = [(kb[ko:ko + kl], vb[vo:vo + vl]) for ko, kl, vo, vl in
               zip(ments["key_off"].tolist(), ments["klen"].tolist(), ments["val_off"].tolist(), ments["vlen"].tolist())]
        assert got == I.entries and mem_bytes == I.mem_bytes, "memtable_build mismatch"
        for k in ("wal_encode_scan_ns", "sst_encode_gather_ns", "mem_validate_ns"):
            assert ctx.get_stat(k) > 0, k
        # four small tables' files against their checksum files
        assert ctx.checksums_verify_many(I.triples) == [0, 0, 0, 0], "checksums_verify_many mismatch"
        for b in bufs:
            b.free()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=3)
    a = ap.parse_args()
    free, secs = [], []
    with tempfile.TemporaryDirectory() as tmp:
        I = Inputs(tmp)
        for _ in range(a.cycles):
            t0 = time.time()
            cycle(I)
            gc.collect()
            torch.cuda.synchronize()
            free.append(int(torch.cuda.mem_get_info(0)[0]))
            secs.append(round(time.time() - t0, 3))
    print(json.dumps({"tool": "ctx_cycle", "cycles": a.cycles, "free_bytes_after_cycle": free,
                      "drop_bytes_last_cycle": free[-2] - free[-1], "cycle_seconds": secs, "results_checked": True}))


if __name__ == "__main__":
    main()
