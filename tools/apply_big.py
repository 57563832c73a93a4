#!/usr/bin/env python3
"""Full-size batch command stream on the GPU (lsmck_db_apply_plan, device form).

tools/write_big.py's stream -- 2^24 config-3 commands (Zipf value lengths,
64 B-64 KiB) with 16-byte keys drawn from --distinct keys (default 2^22), one
in eight a delete -- with every second command replaced by a Get of its key
(a key drawn from the same key set), cut at --limit bytes.  After a warm-up
the call is repeated, alternating with lsmck_db_write_plan over the writes
alone in the same process: every repetition gives the whole call (host clock
around the synchronous call) and its stages between device events
("mem_build_time": order, prep, walk, chain, mark, emit), and the Gets the
memtable answers, a flushed table answers, and the misses.  Yardsticks: that
write plan (what the reads add to the plan), a device-to-device copy of the
command array, and lsmck_db_apply_plan_cpu on the first --cpu commands, whose
segments and Gets are checked equal to the GPU's (a cut and an answer depend on
the commands before them alone).  Writes one JSON line (--out) and prints it.

  python3 tools/apply_big.py [--commands 16777216] [--distinct 4194304] [--limit 4096] [--reps 3] [--out profiles/r16/apply/apply_big_4096.json]
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

STAGES = ("order", "prep", "walk", "chain", "mark", "emit")
WSTAGES = ("order", "walk", "chain", "mark", "emit")


def cpu_apply(keys, cmds, limit):
    """lsmck_db_apply_plan_cpu over the commands: (segs, gets, seconds).  Every
    value range is moved to the start of one small arena of nonzero bytes whose
    last byte is the tombstone's: cuts and answers but val_off stay."""
    n = len(cmds)
    ents, segs = np.empty(n, dtype=_lib.WAL_CMD_DTYPE), np.empty(n + 1, dtype=_lib.WRITE_SEG_DTYPE)
    gets = np.empty(n, dtype=_lib.APPLY_GET_DTYPE)
    moved = cmds.copy()
    moved["val_off"] = 0
    arena = np.ones(int(moved["vlen"][moved["type"] == 1].max(initial=0)) + 1, dtype=np.uint8)
    arena[-1] = 0
    nent, nflush, nget, nmiss, bad = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint64()
    t = time.perf_counter()
    rc = _lib.load().lsmck_db_apply_plan_cpu(keys.ctypes.data, keys.nbytes, arena.ctypes.data, arena.nbytes,
                                             moved.ctypes.data, n, limit, arena.nbytes - 1, ents.ctypes.data, n, None,
                                             segs.ctypes.data, n + 1, gets.ctypes.data, n, None, None, C.byref(nent),
                                             C.byref(nflush), C.byref(nget), C.byref(nmiss), C.byref(bad))
    dt = time.perf_counter() - t
    assert rc == 0, (rc, _lib.last_error())
    return segs[:nflush.value + 1].copy(), gets[:nget.value].copy(), dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commands", type=int, default=1 << 24)
    ap.add_argument("--distinct", type=int, default=1 << 22)
    ap.add_argument("--limit", type=int, default=4096)
    ap.add_argument("--cpu", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "apply", "apply_big_4096.json"))
    a = ap.parse_args()
    n, nd, limit = a.commands, a.distinct, a.limit
    rng = np.random.default_rng(0x5EED0009)
    ln = gen_zipf_lengths(0x5EED0003, n).astype(np.uint64)
    which = rng.integers(0, nd, n).astype(np.uint64)
    types = np.where(rng.integers(0, 8, n) == 0, 2, 1).astype(np.uint32)
    types[1::2] = _lib.CMD_GET  # every second command reads
    vlen = np.where(types == 1, ln - np.minimum(ln, np.uint64(16)), np.uint64(0))
    cmds = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    cmds["type"], cmds["klen"], cmds["vlen"] = types, 16, vlen
    cmds["key_off"] = which * np.uint64(16)
    cmds["val_off"] = np.cumsum(vlen) - vlen
    writes = np.ascontiguousarray(cmds[types != _lib.CMD_GET])
    nw = len(writes)
    h = (np.arange(nd, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nd, 8)
    keys = np.ascontiguousarray(np.concatenate([h, h], axis=1)).ravel()
    kb, vb = keys.nbytes, int(vlen.sum()) + 1  # the value arena and, behind it, the tombstone byte
    tomb = vb - 1
    ng = n - nw
    ctx = Context(0)
    sizes = (kb, vb, cmds.nbytes, writes.nbytes, 32 * nw, 24 * (nw + 1), 24 * ng, 16 * ng, 4 * ng)
    dk, dv, dc, dw, dents, dsegs, dgets, dmq, dmg = (ctx.alloc(max(x, 1)) for x in sizes)
    dk.upload(keys)
    ctx.memset(dv.ptr + tomb, 0, 1)  # (no Insert of one byte is in the stream: no other value byte is read)
    dc.upload(cmds)
    dw.upload(writes)
    ctx.sync()
    ctx.set_option("mem_build_time", 1)
    whole, stages, got = [], {s: [] for s in STAGES}, None
    wwhole, wstages, wgot = [], {s: [] for s in WSTAGES}, None
    for r in range(a.reps + 1):  # the first calls are a warm-up (they allocate the context's scratch)
        t = time.perf_counter()
        got = ctx.db_apply_plan_device(dk.ptr, kb, dv.ptr, vb, dc.ptr, n, limit, tomb, dents.ptr, nw, None, dsegs.ptr,
                                       nw + 1, dgets.ptr, ng, dmq.ptr, dmg.ptr)
        dt = time.perf_counter() - t
        ms = {s: ctx.get_stat(f"apply_{s}_ns") / 1e6 for s in STAGES}
        print(f"apply_plan {r}: {dt * 1e3:.2f} ms, stages {ms}, steps {ctx.get_stat('cut_steps')}, "
              f"long {ctx.get_stat('cut_long')}, (nent, nflush, nget, nmiss) {got}", file=sys.stderr, flush=True)
        if r == a.reps:
            segs = dsegs.download(_lib.WRITE_SEG_DTYPE, got[1] + 1)
            gets = dgets.download(_lib.APPLY_GET_DTYPE, got[2])
            steps, nlong, rounds = ctx.get_stat("cut_steps"), ctx.get_stat("cut_long"), ctx.get_stat("mem_rounds")
        t = time.perf_counter()
        wgot = ctx.db_write_plan_device(dk.ptr, kb, dv.ptr, vb, dw.ptr, nw, limit, tomb, dents.ptr, nw, None, dsegs.ptr,
                                        nw + 1)
        wdt = time.perf_counter() - t
        wms = {s: ctx.get_stat(f"write_{s}_ns") / 1e6 for s in WSTAGES}
        print(f"write_plan {r}: {wdt * 1e3:.2f} ms, stages {wms}, (nent, nflush) {wgot}", file=sys.stderr, flush=True)
        if r:
            whole.append(dt * 1e3)
            wwhole.append(wdt * 1e3)
            for s in STAGES:
                stages[s].append(ms[s])
            for s in WSTAGES:
                wstages[s].append(wms[s])
    nent, nflush, nget, nmiss = got
    assert (nent, nflush) == wgot and nget == ng, "the Gets erased, the plan is the write plan's"
    wsegs = dsegs.download(_lib.WRITE_SEG_DTYPE, nflush + 1)
    assert (wsegs["first_ent"] == segs["first_ent"]).all() and (wsegs["mem_bytes"] == segs["mem_bytes"]).all()
    by_mem = int((gets["source"] == _lib.APPLY_MEMTABLE).sum())
    by_none = int((gets["source"] == _lib.GET_NONE).sum())
    assert by_none == nmiss
    # the check: the prefix's closed segments and its Gets
    m = min(a.cpu, n)
    cpu_segs, cpu_gets, cpu_s = cpu_apply(keys, cmds[:m], limit)
    k = len(cpu_segs) - 1
    assert k <= nflush and (segs["first_cmd"][:k] == cpu_segs["first_cmd"][:k]).all(), "cuts differ from the CPU's"
    assert (segs["mem_bytes"][:k] == cpu_segs["mem_bytes"][:k]).all() and \
        (segs["first_ent"][:k] == cpu_segs["first_ent"][:k]).all()
    g = gets[:len(cpu_gets)]
    assert (g["cmd"] < m).all() and (len(gets) == len(g) or gets["cmd"][len(g)] >= m)
    for f in ("vlen", "source", "cmd", "src_cmd"):
        assert (g[f] == cpu_gets[f]).all(), f"Gets differ from the CPU's in {f}"
    bit = np.uint64(1 << 63)
    assert ((g["val_off"] & bit) == (cpu_gets["val_off"] & bit)).all()
    ins = (g["source"] != _lib.GET_NONE) & ((g["val_off"] & bit) == 0) & (g["vlen"] > 0)
    assert (g["val_off"][ins] == cmds["val_off"][g["src_cmd"][ins]]).all()
    # the yardstick: a device-to-device copy of the commands
    copy = []
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
    for b in (dk, dv, dc, dw, dents, dsegs, dgets, dmq, dmg):
        b.free()
    med = {s: float(np.median(stages[s])) for s in STAGES}
    wmed = {s: float(np.median(wstages[s])) for s in WSTAGES}
    am, wm = float(np.median(whole)), float(np.median(wwhole))
    out = {"metric": "batch command stream of device-resident commands, every second one a Get",
           "value": round(n / 1e6 / (am / 1e3), 1), "unit": "M commands/s", "commands": n, "writes": nw, "gets": nget,
           "distinct_keys": nd, "key_bytes": 16, "limit": limit, "nent": nent, "nflush": nflush,
           "gets_by_memtable": by_mem, "gets_by_table": nget - by_mem - by_none, "gets_missed": by_none,
           "cut_steps": steps, "cut_long": nlong, "mem_rounds": rounds, "reps": a.reps,
           "call_ms_median": round(am, 3), "call_ms_best": round(min(whole), 3),
           "call_ms_all": [round(v, 3) for v in whole], "stage_ms_median": {s: round(med[s], 3) for s in STAGES},
           "stage_ms_all": {s: [round(v, 3) for v in stages[s]] for s in STAGES},
           "bounding_stage": max(STAGES, key=lambda s: med[s]),
           "write_plan_of_the_writes_ms_median": round(wm, 3), "write_plan_of_the_writes_ms_all": [round(v, 3) for v in wwhole],
           "write_plan_stage_ms_median": {s: round(wmed[s], 3) for s in WSTAGES},
           "reads_add_ms": round(am - wm, 3),
           "d2d_copy_commands_ms_median": round(float(np.median(copy)), 3),
           "cpu_apply_commands": m, "cpu_apply_ms": round(cpu_s * 1e3, 3),
           "cpu_apply_mcommands_per_s": round(m / 1e6 / cpu_s, 2), "cpu_prefix_segments_checked": k,
           "cpu_prefix_gets_checked": int(len(cpu_gets))}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
