#!/usr/bin/env python3
"""Full-size batch write plan on the GPU (lsmck_db_write_plan, device form).

tools/memtable_big.py's stream: 2^24 config-3 commands (Zipf value lengths,
64 B-64 KiB) with 16-byte keys drawn from --distinct keys (default 2^22), one
in eight a delete, in random key order -- cut at --limit bytes (the
reference's default memtable_limit_bytes is 4096; 1 MiB is a large one).
After a warm-up the call is repeated; every repetition gives the whole call
(host clock around the synchronous call), its stages between device events
("mem_build_time": order, walk, chain, mark, emit), cut_steps, cut_long and
the segment count.  The closed segments that lie in the first --cpu commands
are checked against lsmck_db_write_plan_cpu over that prefix (a cut depends on
the commands before it alone).  Yardsticks in the same process:
lsmck_memtable_build over the same commands, which shares the sort; a
device-to-device copy of the command array; lsmck_db_write_plan_cpu on the
prefix.  Writes one JSON line (--out) and prints it.

  python3 tools/write_big.py [--commands 16777216] [--distinct 4194304] [--limit 4096] [--reps 3] [--out profiles/r13/write/write_big_4096.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: the torch wheel's HIP runtime)
from lsm_storage_engine_amd import _lib  # noqa: E402
from lsm_storage_engine_amd.device import Context, gen_zipf_lengths  # noqa: E402

STAGES = ("order", "walk", "chain", "mark", "emit")


def cpu_plan(keys, cmds, limit):
    """lsmck_db_write_plan_cpu over the commands: (segs, seconds).  A cut
    depends on the keys and the lengths alone, so every value range is moved
    to the start of one small arena whose last byte is the tombstone's."""
    n = len(cmds)
    ents, segs = np.empty(n, dtype=_lib.WAL_CMD_DTYPE), np.empty(n + 1, dtype=_lib.WRITE_SEG_DTYPE)
    moved = cmds.copy()
    moved["val_off"] = 0
    arena = np.zeros(int(moved["vlen"][moved["type"] == 1].max(initial=0)) + 1, dtype=np.uint8)
    nent, nflush, bad = C.c_size_t(), C.c_size_t(), C.c_uint64()
    t = time.perf_counter()
    rc = _lib.load().lsmck_db_write_plan_cpu(keys.ctypes.data, keys.nbytes, arena.ctypes.data, arena.nbytes,
                                             moved.ctypes.data, n, limit, arena.nbytes - 1, ents.ctypes.data, n, None,
                                             segs.ctypes.data, n + 1, C.byref(nent), C.byref(nflush), C.byref(bad))
    dt = time.perf_counter() - t
    assert rc == 0, (rc, _lib.last_error())
    return segs[:nflush.value + 1].copy(), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commands", type=int, default=1 << 24)
    ap.add_argument("--distinct", type=int, default=1 << 22)
    ap.add_argument("--limit", type=int, default=4096)
    ap.add_argument("--cpu", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "write", "write_big_4096.json"))
    a = ap.parse_args()
    n, nd, limit = a.commands, a.distinct, a.limit
    rng = np.random.default_rng(0x5EED0009)
    ln = gen_zipf_lengths(0x5EED0003, n).astype(np.uint64)
    which = rng.integers(0, nd, n).astype(np.uint64)
    types = np.where(rng.integers(0, 8, n) == 0, 2, 1).astype(np.uint32)
    vlen = np.where(types == 1, ln - np.minimum(ln, np.uint64(16)), np.uint64(0))
    cmds = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    cmds["type"], cmds["klen"], cmds["vlen"] = types, 16, vlen
    cmds["key_off"] = which * np.uint64(16)
    cmds["val_off"] = np.cumsum(vlen) - vlen
    h = (np.arange(nd, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nd, 8)
    keys = np.ascontiguousarray(np.concatenate([h, h], axis=1)).ravel()
    kb, vb = keys.nbytes, int(vlen.sum()) + 1  # the value arena and, behind it, the tombstone byte
    tomb = vb - 1
    ctx = Context(0)
    dk, dv, dc, dents, dsegs = (ctx.alloc(x) for x in (kb, vb, cmds.nbytes, 32 * n, 24 * (n + 1)))
    dk.upload(keys)
    ctx.memset(dv.ptr + tomb, 0, 1)  # (no other value byte is read by the plan)
    dc.upload(cmds)
    ctx.sync()
    ctx.set_option("mem_build_time", 1)
    whole, stages, got = [], {s: [] for s in STAGES}, None
    for r in range(a.reps + 1):  # the first call is a warm-up (it allocates the context's scratch)
        t = time.perf_counter()
        got = ctx.db_write_plan_device(dk.ptr, kb, dv.ptr, vb, dc.ptr, n, limit, tomb, dents.ptr, n, None, dsegs.ptr,
                                       n + 1)
        dt = time.perf_counter() - t
        ms = {s: ctx.get_stat(f"write_{s}_ns") / 1e6 for s in STAGES}
        print(f"write_plan {r}: {dt * 1e3:.2f} ms, stages {ms}, steps {ctx.get_stat('cut_steps')}, "
              f"long {ctx.get_stat('cut_long')}, (nent, nflush) {got}", file=sys.stderr, flush=True)
        if r:
            whole.append(dt * 1e3)
            for s in STAGES:
                stages[s].append(ms[s])
    steps, nlong, rounds = ctx.get_stat("cut_steps"), ctx.get_stat("cut_long"), ctx.get_stat("mem_rounds")
    nent, nflush = got
    segs = dsegs.download(_lib.WRITE_SEG_DTYPE, nflush + 1)
    # the check: the prefix's closed segments
    m = min(a.cpu, n)
    cpu_segs, cpu_s = cpu_plan(keys, cmds[:m], limit)
    k = len(cpu_segs) - 1
    assert k <= nflush and (segs["first_cmd"][:k] == cpu_segs["first_cmd"][:k]).all(), "cuts differ from the CPU's"
    assert (segs["mem_bytes"][:k] == cpu_segs["mem_bytes"][:k]).all() and \
        (segs["first_ent"][:k] == cpu_segs["first_ent"][:k]).all()
    # the yardsticks: the memtable build over the same commands, a device-to-device copy of the commands
    build, copy = [], []
    for r in range(a.reps + 1):
        t = time.perf_counter()
        ctx.memtable_build_device(dk.ptr, kb, dv.ptr, vb, dc.ptr, n, dents.ptr, n, None)
        if r:
            build.append((time.perf_counter() - t) * 1e3)
    x = torch.empty(cmds.nbytes, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        if r:
            copy.append(e0.elapsed_time(e1))
    ctx.set_option("mem_build_time", 0)
    for b in (dk, dv, dc, dents, dsegs):
        b.free()
    med = {s: float(np.median(stages[s])) for s in STAGES}
    wm = float(np.median(whole))
    out = {"metric": "batch write plan of device-resident commands (order + walk + chain + mark + emit)",
           "value": round(n / 1e6 / (wm / 1e3), 1), "unit": "M commands/s", "commands": n, "distinct_keys": nd,
           "key_bytes": 16, "limit": limit, "nent": nent, "nflush": nflush,
           "commands_per_segment": round(n / (nflush + 1), 2), "cut_steps": steps, "cut_long": nlong,
           "mem_rounds": rounds, "reps": a.reps, "call_ms_median": round(wm, 3), "call_ms_best": round(min(whole), 3),
           "call_ms_all": [round(v, 3) for v in whole], "stage_ms_median": {s: round(med[s], 3) for s in STAGES},
           "stage_ms_all": {s: [round(v, 3) for v in stages[s]] for s in STAGES},
           "bounding_stage": max(STAGES, key=lambda s: med[s]),
           "memtable_build_ms_median": round(float(np.median(build)), 3),
           "d2d_copy_commands_ms_median": round(float(np.median(copy)), 3),
           "cpu_plan_commands": m, "cpu_plan_ms": round(cpu_s * 1e3, 3),
           "cpu_plan_mcommands_per_s": round(m / 1e6 / cpu_s, 2), "cpu_prefix_segments_checked": k}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
