#!/usr/bin/env python3
"""Full-size batch SSTable encode on the GPU (lsmck_sstable_encode_batch, device form).

Config 3's Zipf payloads (64 B-64 KiB, 2^24 of them by default: about 24 GiB)
as entries with a 16-byte key split -- sorted keys in one device arena, values
in another -- cut into tables of about 4 KiB * 4^level with
tree.synthesize_tree's level shares of the bytes, encoded into a
device-resident data arena and index arena with both digests per table.
After a warm-up the call is repeated; every repetition gives the whole call
(host clock around the synchronous call) and its stages between device events
("sst_encode_time": sizes / order / index plan / spans, the data gather, the
index writer, the digests).  Two yardsticks run in the same process: a
hipMemcpyAsync device-to-device copy of the data arena's byte count (the same
bytes, no search, no realignment), and lsmck_wal_encode_batch over the same
entries ("wal_encode_time": its gather).  The first and last tables are read
back and compared with hashlib.  Writes one JSON line (--out) and prints it.

  python3 tools/sst_encode_big.py [--records 16777216] [--reps 3] [--out profiles/r08/sstenc/sst_encode_big.json]
"""
import argparse
import ctypes as C
import hashlib
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
STAGES = ("scan", "gather", "index", "sha")
WAL_STAGES = ("scan", "gather", "crc", "stamp")
SHARE = (0.001, 0.004, 0.025, 0.12, 0.85)  # tree.synthesize_tree's share of the bytes per level


def cut_tables(size, seed=0x5EED0005):
    """table_first for records of `size` bytes each: level lv's share of the
    bytes in tables of about 4 KiB * 4^lv (x 0.75 .. 1.25), level 0 first."""
    rng = np.random.default_rng(seed)
    end = np.cumsum(size).astype(np.int64)  # (searched with int64 needles: no conversion of the array per search)
    total, n = int(end[-1]), len(size)
    cuts, at = [0], 0
    for lv, share in enumerate(SHARE):
        stop = total if lv == len(SHARE) - 1 else at + int(total * share)
        while at < stop and cuts[-1] < n:
            at += int((4096 << (2 * lv)) * rng.uniform(0.75, 1.25))
            cuts.append(max(cuts[-1] + 1, min(n, int(np.searchsorted(end, np.int64(min(at, stop)), side="right")))))
    if cuts[-1] < n:
        cuts.append(n)
    return np.array(cuts, dtype=np.uint64)


def median_stages(ctx, prefix, names, call, reps):
    whole, stages = [], {s: [] for s in names}
    for r in range(reps + 1):  # the first call is a warm-up (it allocates the context's scratch)
        t = time.perf_counter()
        call()
        dt = time.perf_counter() - t
        ms = {s: ctx.get_stat(f"{prefix}_{s}_ns") / 1e6 for s in names}
        print(f"{prefix} {r}: {dt * 1e3:.2f} ms, stages {ms}", file=sys.stderr, flush=True)
        if r:
            whole.append(dt * 1e3)
            for s in names:
                stages[s].append(ms[s])
    return whole, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r08", "sstenc", "sst_encode_big.json"))
    a = ap.parse_args()
    n = a.records
    ln = gen_zipf_lengths(0x5EED0003, n).astype(np.uint64)
    klen = np.minimum(ln, np.uint64(16))
    vlen = ln - klen
    ents = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    ents["type"], ents["klen"], ents["vlen"] = 1, klen, vlen
    ents["key_off"] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    ents["val_off"] = np.cumsum(vlen) - vlen
    size = np.uint64(8) + klen + vlen
    first = cut_tables(size)
    ntab = len(first) - 1
    ctx = Context(0)
    db, ib = C.c_uint64(), C.c_uint64()
    assert ctx.lib.lsmck_sstable_encoded_size(ents.ctypes.data, n, first.ctypes.data, ntab, C.byref(db),
                                              C.byref(ib)) == 0
    total, itotal, kb, vb = db.value, ib.value, 16 * n, int(vlen.sum())
    assert total == int(size.sum())
    # sorted 16-byte keys: the entry's number, big-endian, twice
    be = np.arange(n, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    keys = np.ascontiguousarray(np.concatenate([be, be], axis=1)).ravel()
    dk, dv, de = (ctx.alloc(x) for x in (kb, max(vb, 1), ents.nbytes))
    dk.upload(keys)
    ctx.gen_stream(dv.ptr, 0x5EED00A2, 0, vb)
    de.upload(ents)
    ddata, dindex, dspans, dsha = (ctx.alloc(x) for x in (total, itotal, 32 * ntab, 64 * ntab))
    ctx.sync()
    ctx.set_option("sst_encode_time", 1)
    whole, stages = median_stages(ctx, "sst_encode", STAGES, lambda: ctx.sstable_encode_batch_device(
        dk.ptr, kb, dv.ptr, vb, de.ptr, n, first, ddata.ptr, total, dindex.ptr, itotal, dspans.ptr, dsha.ptr,
        dsha.ptr + 32 * ntab), a.reps)
    ctx.set_option("sst_encode_time", 0)
    # what was built: the first and the last table against hashlib
    spans = dspans.download(_lib.SSTABLE_SPAN_DTYPE, ntab)
    sha = dsha.download().reshape(2, ntab, 32)
    assert int(spans[-1]["data_off"] + spans[-1]["data_len"]) == total
    assert int(spans[-1]["index_off"] + spans[-1]["index_len"]) == itotal
    for t in (0, ntab - 1):
        d = ddata.download(np.uint8, int(spans[t]["data_len"]), int(spans[t]["data_off"]))
        x = dindex.download(np.uint8, int(spans[t]["index_len"]), int(spans[t]["index_off"]))
        assert hashlib.sha256(d.tobytes()).digest() == sha[0, t].tobytes(), t
        assert hashlib.sha256(x.tobytes()).digest() == sha[1, t].tobytes(), t
        assert int.from_bytes(x[:8].tobytes(), "little") == (int(first[t + 1] - first[t]) + 99) // 100
    tile = ctx.get_stat("sst_encode_tile")
    for b in (ddata, dindex, dspans, dsha):
        b.free()
    # yardstick 2: the WAL encode of the same entries (Inserts), its gather
    wal_total = int((np.uint64(13) + klen + vlen).sum())
    dimg = ctx.alloc(wal_total)
    ctx.set_option("wal_encode_time", 1)
    _, wal_stages = median_stages(ctx, "wal_encode", WAL_STAGES, lambda: ctx.wal_encode_batch_device(
        dk.ptr, kb, dv.ptr, vb, de.ptr, n, dimg.ptr, wal_total), a.reps)
    ctx.set_option("wal_encode_time", 0)
    for b in (dk, dv, de, dimg):
        b.free()
    # yardstick 1: hipMemcpyAsync device to device, the data arena's byte count
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    src.fill_(0x5A)
    ts = []
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)  # same dtype, contiguous: hipMemcpyAsync(hipMemcpyDeviceToDevice)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    copy_ms = float(np.median(ts))
    med = {s: float(np.median(stages[s])) for s in STAGES}
    wal_gather = float(np.median(wal_stages["gather"]))
    wm = float(np.median(whole))
    out = {"metric": "batch SSTable encode of device-resident entries (scan + gather + index + digests)",
           "value": round(total / GIB / (wm / 1e3), 1), "unit": "GiB/s of data files", "data_bytes": total,
           "index_bytes": itotal, "entries": n, "tables": ntab, "reps": a.reps, "tile_bytes": tile,
           "records_per_tile": round(n * tile / total, 1),
           "call_ms_median": round(wm, 3), "call_ms_best": round(min(whole), 3),
           "stage_ms_median": {s: round(med[s], 3) for s in STAGES},
           "stage_ms_all": {s: [round(x, 3) for x in stages[s]] for s in STAGES},
           "gather_gib_s": round(total / GIB / (med["gather"] / 1e3), 1),
           "copy_d2d_ms_median": round(copy_ms, 3), "copy_d2d_ms_all": [round(x, 3) for x in ts],
           "copy_d2d_gib_s": round(total / GIB / (copy_ms / 1e3), 1),
           "gather_share_of_copy": round(copy_ms / med["gather"], 3),
           "wal_log_bytes": wal_total, "wal_gather_ms_median": round(wal_gather, 3),
           "wal_gather_ms_all": [round(x, 3) for x in wal_stages["gather"]],
           "wal_gather_share_of_copy": round(copy_ms * (wal_total / total) / wal_gather, 3),
           "gather_ns_per_byte_over_wal_gather": round((med["gather"] / total) / (wal_gather / wal_total), 3)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
