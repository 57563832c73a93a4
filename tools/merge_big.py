#!/usr/bin/env python3
"""Full-size batch compaction on the GPU: lsmck_sstable_decode_batch,
lsmck_sstable_merge_batch and lsmck_sstable_encode_batch, device form.

Config 3's Zipf value lengths (capped by --kmax so that a table's data file
stays under the decode's 2^32-1 bytes) as entries with 16-byte keys, in two
shapes:
  one   one group of 4 tables of 2^22 entries over 2^22 distinct keys;
  many  4,096 groups of 4 tables of 1,024 entries (half of a group's keys shared).
The tables' data and index images are built on the device by the encode (setup,
not timed).  Then every stage is timed between device events
("sst_encode_time"): the decode's index walk, segment walks, counts / scans and
emit; the merge's order keys, shadow, scan and place; and the encode of the
merged run.  Yardsticks in the same process: for the decode a device-to-device
hipMemcpyAsync of the data arena's bytes (the floor for touching the images)
and the plain walk (index = NULL: one lane per table); for the merge of shape
`one` lsmck_memtable_build over the same decoded entries as Inserts in table
order -- the only other way in the library to the same run -- whose output must
equal the merge's (asserted).  Writes one JSON line (--out) and prints it.

  python3 tools/merge_big.py [--log2 22] [--groups 4096] [--reps 3] [--out profiles/r10/merge/merge_big.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library: the torch wheel's HIP runtime)
from lsm_storage_engine_amd import _lib  # noqa: E402
from lsm_storage_engine_amd.device import Context, gen_zipf_lengths  # noqa: E402

GIB = float(1 << 30)
DEC = ("index", "seg", "scan", "emit")
MRG = ("okey", "shadow", "scan", "place")
ENC = ("scan", "gather", "index", "sha")
MEM = ("validate", "chunk", "sort", "resolve")


def timed(ctx, prefix, names, call, reps):
    """Medians over `reps` calls after a warm-up: (whole call ms, {stage: ms})."""
    whole, stages = [], {s: [] for s in names}
    for r in range(reps + 1):
        t = time.perf_counter()
        call()
        dt = (time.perf_counter() - t) * 1e3
        ms = {s: ctx.get_stat(f"{prefix}_{s}_ns") / 1e6 for s in names}
        print(f"{prefix} {r}: {dt:.2f} ms, stages {ms}", file=sys.stderr, flush=True)
        if r:
            whole.append(dt)
            for s in names:
                stages[s].append(ms[s])
    return round(float(np.median(whole)), 3), {s: round(float(np.median(v)), 3) for s, v in stages.items()}


def copy_d2d_ms(nbytes, reps):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.fill_(0x5A)
    ts = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)  # same dtype, contiguous: hipMemcpyAsync(hipMemcpyDeviceToDevice)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    del src, dst
    return round(float(np.median(ts)), 3)


def shape(ctx, name, ngrp, m, shared_all, kmax, reps, digests, sort_yardstick):
    """ngrp groups of 4 tables of m entries."""
    ntab, n = 4 * ngrp, 4 * ngrp * m
    ln = gen_zipf_lengths(0x5EED0003, n, kmax=kmax).astype(np.uint64)
    vlen = ln - np.uint64(16)  # (lmin = 64: a 16-byte key and the rest)
    i = np.tile(np.arange(m, dtype=np.uint64), ntab)
    t = np.repeat(np.arange(ntab, dtype=np.uint64) % np.uint64(4), m)
    ids = i if shared_all else np.uint64(2) * i + ((i >> t) & np.uint64(1))
    be = ids.astype(">u8").view(np.uint8).reshape(n, 8)
    keys = np.ascontiguousarray(np.concatenate([be, be], axis=1)).ravel()
    ents = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    ents["type"], ents["klen"], ents["vlen"] = 1, 16, vlen
    ents["key_off"] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    ents["val_off"] = np.cumsum(vlen) - vlen
    first = np.arange(ntab + 1, dtype=np.uint64) * np.uint64(m)
    group_first = np.arange(ngrp + 1, dtype=np.uint64) * np.uint64(4)
    kb, vb = 16 * n, int(vlen.sum())
    db, ib = n * 24 + vb, ntab * 8 + ntab * ((m + 99) // 100) * 32
    # setup: the old tables' images, by the encode
    dk, dv, de = ctx.alloc(kb), ctx.alloc(max(vb, 1)), ctx.alloc(ents.nbytes)
    dk.upload(keys)
    ctx.gen_stream(dv.ptr, 0x5EED00A2, 0, vb)
    de.upload(ents)
    ddata, dindex, dspans = ctx.alloc(db), ctx.alloc(ib), ctx.alloc(32 * ntab)
    assert ctx.sstable_encode_batch_device(dk.ptr, kb, dv.ptr, vb, de.ptr, n, first, ddata.ptr, db, dindex.ptr, ib,
                                           dspans.ptr) == (db, ib)
    for b in (dk, dv):
        b.free()
    out = {"shape": name, "groups": ngrp, "tables": ntab, "entries": n, "data_bytes": db, "index_bytes": ib}
    # decode: with the index as the hint, and plainly
    dents, dcons = ctx.alloc(32 * n), ctx.alloc(8 * ntab)
    ctx.set_option("sst_encode_time", 1)
    res = {}

    def decode(index):
        res["dec"] = ctx.sstable_decode_batch_device(ddata.ptr, db, dindex.ptr if index else None, ib, dspans.ptr, ntab,
                                                     dents.ptr, n, dcons.ptr)
    out["decode_ms"], out["decode_stage_ms"] = timed(ctx, "sst_decode", DEC, lambda: decode(True), reps)
    assert ctx.get_stat("sst_decode_declined") == 0 and res["dec"][0] == n
    out["decode_uniform_tables"] = ctx.get_stat("sst_decode_uniform")  # (16-byte keys: every index is proven in parallel)
    assert res["dec"][1].tolist() == first.tolist()
    assert np.array_equal(dcons.download(np.uint64), (np.uint64(24) + vlen).reshape(ntab, m).sum(axis=1))
    hinted = dents.download(_lib.WAL_CMD_DTYPE, n)
    assert np.array_equal(hinted["klen"], ents["klen"]) and np.array_equal(hinted["vlen"], ents["vlen"])
    t0 = time.perf_counter()
    decode(False)
    out["decode_plain_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert dents.download(_lib.WAL_CMD_DTYPE, n).tobytes() == hinted.tobytes()
    del hinted
    out["copy_d2d_ms"] = copy_d2d_ms(db, reps)
    out["decode_over_copy"] = round(out["decode_ms"] / out["copy_d2d_ms"], 2)
    # merge
    dout, dsrc = ctx.alloc(32 * n), ctx.alloc(4 * n)

    def merge():
        res["mrg"] = ctx.sstable_merge_batch_device(ddata.ptr, db, ddata.ptr, db, dents.ptr, n, first, group_first,
                                                    dout.ptr, n, dsrc.ptr, tombstones="keep")
    out["merge_ms"], out["merge_stage_ms"] = timed(ctx, "sst_merge", MRG, merge, reps)
    nout, out_first = res["mrg"]
    out["winners"] = nout
    low = np.arange(m) & 15  # (shape `many`: key 2i + bit t of i -- both keys of a pair unless i's low 4 bits agree)
    assert nout == ngrp * (m if shared_all else int(np.where((low == 0) | (low == 15), 1, 2).sum()))
    if sort_yardstick:  # the sort route: the same entries as Inserts in table order, the last writer wins
        dents2, dsrc2 = ctx.alloc(32 * n), ctx.alloc(4 * n)
        ctx.set_option("mem_build_time", 1)
        out["memtable_build_ms"], out["memtable_build_stage_ms"] = timed(
            ctx, "mem", MEM, lambda: ctx.memtable_build_device(ddata.ptr, db, ddata.ptr, db, dents.ptr, n, dents2.ptr, n,
                                                               dsrc2.ptr), reps)
        ctx.set_option("mem_build_time", 0)
        assert dents2.download(_lib.WAL_CMD_DTYPE, nout).tobytes() == dout.download(_lib.WAL_CMD_DTYPE, nout).tobytes()
        assert dsrc2.download(np.uint32, nout).tobytes() == dsrc.download(np.uint32, nout).tobytes()
        out["merge_over_memtable_build"] = round(out["merge_ms"] / out["memtable_build_ms"], 3)
        dents2.free()
        dsrc2.free()
    # encode of the merged run (a table is one sequential SHA-256: digests only where tables are small)
    # the encode's size query: with no buffers it writes nothing and reports LSMCK_ENOSPC with both sizes
    try:
        ctx.sstable_encode_batch_device(ddata.ptr, db, ddata.ptr, db, dout.ptr, nout, out_first, None, 0, None, 0)
        raise AssertionError("an index file is never empty")
    except _lib.LsmckError as e:
        ndb, nib = e.needed
    nd, nx, nsha = ctx.alloc(ndb), ctx.alloc(nib), ctx.alloc(64 * ngrp)
    out["encode_ms"], out["encode_stage_ms"] = timed(ctx, "sst_encode", ENC, lambda: ctx.sstable_encode_batch_device(
        ddata.ptr, db, ddata.ptr, db, dout.ptr, nout, out_first, nd.ptr, ndb, nx.ptr, nib, None,
        nsha.ptr if digests else None, nsha.ptr + 32 * ngrp if digests else None), reps)
    out["encode_digests"] = bool(digests)
    out["out_data_bytes"] = ndb
    ctx.set_option("sst_encode_time", 0)
    for b in (de, ddata, dindex, dspans, dents, dcons, dout, dsrc, nd, nx, nsha):
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=22, help="shape `one`: entries per table")
    ap.add_argument("--groups", type=int, default=4096, help="shape `many`: groups of 4 tables of 1,024 entries")
    ap.add_argument("--kmax", type=int, default=64, help="Zipf lengths on k = 1..kmax (L = 64k - j)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "merge", "merge_big.json"))
    a = ap.parse_args()
    ctx = Context(0)
    out = {"metric": "batch compaction on the device: decode, merge, encode (stage times between device events)",
           "kmax": a.kmax, "reps": a.reps,
           "one": shape(ctx, "one", 1, 1 << a.log2, True, a.kmax, a.reps, False, True),
           "many": shape(ctx, "many", a.groups, 1024, False, a.kmax, a.reps, True, False)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
