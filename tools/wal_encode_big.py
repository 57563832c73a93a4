#!/usr/bin/env python3
"""Full-size batch WAL encode on the GPU (lsmck_wal_encode_batch, device form).

Config 3's Zipf payloads (64 B-64 KiB, 2^24 of them by default: about 24 GiB)
as Insert commands with a 16-byte key split -- keys in one device arena,
values in another -- encoded into a device-resident log.  After a warm-up the
call is repeated; every repetition gives the whole call (host clock around the
synchronous call: it reads the total back in the middle) and its stages
between device events ("wal_encode_time": size / validate / scan, gather,
descriptors + CRC pass, stamp).  In the same process a hipMemcpyAsync
device-to-device copy of the image's byte count is timed between device events
too: the gather's yardstick (the same bytes, no search, no realignment).  The
log is then replayed (lsmck_wal_replay_verify: status 0, every record) and the
record offsets compared with the host's prefix sums.  Prints one JSON line.

  python3 tools/wal_encode_big.py [--records 16777216] [--reps 5] [--removes 0] [--lmin 64]
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
STAGES = ("scan", "gather", "crc", "stamp")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--removes", type=int, default=0, help="N: every Nth command is a Remove of its key (0: none)")
    ap.add_argument("--copy", type=int, default=1, help="0: skip the device-to-device copy yardstick")
    ap.add_argument("--lmin", type=int, default=64,
                    help="the shortest payload (config 3: 64); 65536 makes every payload 64 KiB: a log with "
                         "hardly a chunk on a record boundary (A/B of the gather's bytewise path)")
    a = ap.parse_args()
    n = a.records
    ln = gen_zipf_lengths(0x5EED0003, n, lmin=a.lmin).astype(np.uint64)
    cmds = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    klen = np.minimum(ln, np.uint64(16))
    ins = np.ones(n, bool) if not a.removes else (np.arange(n) % a.removes != a.removes - 1)
    vlen = np.where(ins, ln - klen, np.uint64(0))
    cmds["type"] = np.where(ins, 1, 2)
    cmds["klen"], cmds["vlen"] = klen, vlen
    cmds["key_off"] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    cmds["val_off"] = np.cumsum(vlen) - vlen
    size = np.where(ins, 13, 9).astype(np.uint64) + klen + vlen
    off = np.cumsum(size) - size
    total, kb, vb = int(size.sum()), 16 * n, int(vlen.sum())
    ctx = Context(0)
    assert ctx.lib.lsmck_wal_encoded_size(cmds.ctypes.data, n) == total
    dk, dv, dc, drec, dimg = (ctx.alloc(x) for x in (kb, max(vb, 1), cmds.nbytes, 8 * n, total))
    ctx.gen_stream(dk.ptr, 0x5EED00A1, 0, kb)
    ctx.gen_stream(dv.ptr, 0x5EED00A2, 0, vb)
    dc.upload(cmds)
    ctx.sync()
    ctx.set_option("wal_encode_time", 1)
    whole, stages = [], {s: [] for s in STAGES}
    for r in range(a.reps + 1):  # the first call is a warm-up (it allocates the context's scratch)
        t = time.perf_counter()
        got = ctx.wal_encode_batch_device(dk.ptr, kb, dv.ptr, vb, dc.ptr, n, dimg.ptr, total, drec.ptr)
        dt = time.perf_counter() - t
        assert got == total
        ms = {s: ctx.get_stat(f"wal_encode_{s}_ns") / 1e6 for s in STAGES}
        print(f"encode {r}: {dt * 1e3:.2f} ms, stages {ms}", file=sys.stderr, flush=True)
        if r:
            whole.append(dt)
            for s in STAGES:
                stages[s].append(ms[s])
    ctx.set_option("wal_encode_time", 0)
    # what was built: the log replays clean, every record where the prefix sums say
    recs, status, bad = ctx.wal_replay_verify(total, device_ptr=dimg.ptr, cap=1)
    assert status == 0, (status, bad)
    assert np.array_equal(drec.download(np.uint64, n), off)
    tile = ctx.get_stat("wal_encode_tile")
    for b in (dk, dv, dc, drec):
        b.free()
    copy_ms = None
    if a.copy:  # the yardstick: hipMemcpyAsync device to device, the image's byte count
        dimg.free()
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
    wm = float(np.median(whole)) * 1e3
    gather_rate = total / GIB / (med["gather"] / 1e3)
    out = {"metric": "batch WAL encode of device-resident commands (scan + gather + CRC pass + stamp)",
           "value": round(total / GIB / (wm / 1e3), 1), "unit": "GiB/s of log", "log_bytes": total, "records": n,
           "removes_every": a.removes, "lmin": a.lmin, "reps": a.reps, "tile_bytes": tile,
           "call_ms_median": round(wm, 3), "call_ms_best": round(min(whole) * 1e3, 3),
           "stage_ms_median": {s: round(med[s], 3) for s in STAGES},
           "stage_ms_all": {s: [round(x, 3) for x in stages[s]] for s in STAGES},
           "gather_gib_s": round(gather_rate, 1),
           "copy_d2d_ms_median": None if copy_ms is None else round(copy_ms, 3),
           "copy_d2d_gib_s": None if copy_ms is None else round(total / GIB / (copy_ms / 1e3), 1),
           "gather_share_of_copy": None if copy_ms is None else round(copy_ms / med["gather"], 3),
           "replay_status": status}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
