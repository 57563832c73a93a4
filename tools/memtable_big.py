#!/usr/bin/env python3
"""Full-size batch memtable build on the GPU (lsmck_memtable_build, device form).

2^24 config-3 commands (Zipf value lengths, 64 B-64 KiB) with 16-byte keys
drawn from --distinct keys (default 2^22, so three of four commands overwrite
an earlier one), one in eight a Remove, in random key order: the arrival order
of a group commit or of a log replayed on the GPU.  After a warm-up the build
is repeated; every repetition gives the whole call (host clock around the
synchronous call), its stages between device events ("mem_build_time":
validate, the kernel that reads key bytes, the rounds' fixed-width part,
resolve / emit) and the rounds.  nent and mem_bytes are checked against numpy.
The live entries then go to lsmck_sstable_encode_batch as they are, in tables
of 2^16 entries.  Yardstick in the same process: torch.sort(stable=True) of n
int64 keys on the same device -- one fixed-width sort of the batch, which any
sort-based build pays at least once.  Writes one JSON line (--out) and prints it.

  python3 tools/memtable_big.py [--commands 16777216] [--distinct 4194304] [--reps 3] [--out profiles/r09/memtable/memtable_big.json]
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

STAGES = ("validate", "chunk", "sort", "resolve")


def expected(which, types, size):
    """(nent, mem_bytes) of the log by numpy: the commands in (key, position)
    order; a key's last command when it is an Insert; the Inserts' sizes less,
    for a Remove behind an Insert of its key, that Insert's size."""
    order = np.argsort(which, kind="stable")
    w, t, s = which[order], types[order], size[order].astype(np.int64)
    last = np.ones(len(w), dtype=bool)
    last[:-1] = w[1:] != w[:-1]
    nent = int((last & (t == 1)).sum())
    takes = np.zeros(len(w), dtype=bool)
    takes[1:] = (t[1:] == 2) & (w[1:] == w[:-1]) & (t[:-1] == 1)
    return nent, int(s[t == 1].sum() - s[:-1][takes[1:]].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commands", type=int, default=1 << 24)
    ap.add_argument("--distinct", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "memtable", "memtable_big.json"))
    a = ap.parse_args()
    n, nd = a.commands, a.distinct
    rng = np.random.default_rng(0x5EED0009)
    ln = gen_zipf_lengths(0x5EED0003, n).astype(np.uint64)
    which = rng.integers(0, nd, n).astype(np.uint64)
    types = np.where(rng.integers(0, 8, n) == 0, 2, 1).astype(np.uint32)
    vlen = np.where(types == 1, ln - np.minimum(ln, np.uint64(16)), np.uint64(0))
    cmds = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    cmds["type"], cmds["klen"], cmds["vlen"] = types, 16, vlen
    cmds["key_off"] = which * np.uint64(16)
    cmds["val_off"] = np.cumsum(vlen) - vlen
    # key id -> 16 bytes: a bijective scramble of the id, big-endian, twice (key order is not id order)
    h = (np.arange(nd, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(nd, 8)
    keys = np.ascontiguousarray(np.concatenate([h, h], axis=1)).ravel()
    kb, vb = keys.nbytes, int(vlen.sum())
    want_nent, want_bytes = expected(which, types, np.uint64(16) + vlen)
    ctx = Context(0)
    dk, dv, dc, dents, dsrc = (ctx.alloc(x) for x in (kb, max(vb, 1), cmds.nbytes, 32 * n, 4 * n))
    dk.upload(keys)
    ctx.gen_stream(dv.ptr, 0x5EED00A2, 0, vb)
    dc.upload(cmds)
    ctx.sync()
    ctx.set_option("mem_build_time", 1)
    whole, stages, got = [], {s: [] for s in STAGES}, None
    for r in range(a.reps + 1):  # the first call is a warm-up (it allocates the context's scratch)
        t = time.perf_counter()
        got = ctx.memtable_build_device(dk.ptr, kb, dv.ptr, vb, dc.ptr, n, dents.ptr, n, dsrc.ptr)
        dt = time.perf_counter() - t
        ms = {s: ctx.get_stat(f"mem_{s}_ns") / 1e6 for s in STAGES}
        print(f"mem_build {r}: {dt * 1e3:.2f} ms, stages {ms}, rounds {ctx.get_stat('mem_rounds')}", file=sys.stderr,
              flush=True)
        if r:
            whole.append(dt * 1e3)
            for s in STAGES:
                stages[s].append(ms[s])
    ctx.set_option("mem_build_time", 0)
    rounds = ctx.get_stat("mem_rounds")
    assert got == (want_nent, want_bytes), (got, want_nent, want_bytes)
    nent = got[0]
    # the result feeds the SSTable encode as it is: tables of 2^16 entries
    first = np.unique(np.concatenate([np.arange(0, nent, 1 << 16), [nent]])).astype(np.uint64)
    ntab = len(first) - 1
    src = dsrc.download(np.uint32, nent)
    data_bytes = int((np.uint64(8 + 16) + vlen[src]).sum())
    index_bytes = int(sum(8 + 32 * ((int(first[t + 1] - first[t]) + 99) // 100) for t in range(ntab)))
    ddata, dindex, dsha = (ctx.alloc(x) for x in (max(data_bytes, 1), index_bytes, 64 * ntab))
    t = time.perf_counter()
    enc = ctx.sstable_encode_batch_device(dk.ptr, kb, dv.ptr, vb, dents.ptr, nent, first, ddata.ptr, data_bytes,
                                          dindex.ptr, index_bytes, None, dsha.ptr, dsha.ptr + 32 * ntab)
    sst_ms = (time.perf_counter() - t) * 1e3
    assert enc == (data_bytes, index_bytes), (enc, data_bytes, index_bytes)
    for b in (dk, dv, dc, dents, dsrc, ddata, dindex, dsha):
        b.free()
    # the yardstick: one stable sort of n int64 keys
    x = torch.from_numpy(which.astype(np.int64)).cuda()
    ts = []
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.sort(x, stable=True)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    sort_ms = float(np.median(ts))
    med = {s: float(np.median(stages[s])) for s in STAGES}
    wm = float(np.median(whole))
    out = {"metric": "batch memtable build of device-resident commands (validate + rounds + resolve + emit)",
           "value": round(n / 1e6 / (wm / 1e3), 1), "unit": "M commands/s", "commands": n, "distinct_keys": nd,
           "key_bytes": 16, "nent": nent, "mem_bytes": got[1], "mem_rounds": rounds, "reps": a.reps,
           "call_ms_median": round(wm, 3), "call_ms_best": round(min(whole), 3),
           "call_ms_all": [round(v, 3) for v in whole],
           "stage_ms_median": {s: round(med[s], 3) for s in STAGES},
           "stage_ms_all": {s: [round(v, 3) for v in stages[s]] for s in STAGES},
           "torch_sort_stable_int64_ms_median": round(sort_ms, 3), "torch_sort_ms_all": [round(v, 3) for v in ts],
           "call_over_torch_sort": round(wm / sort_ms, 2),
           "sst_encode_after_ms": round(sst_ms, 3), "sst_tables": ntab, "sst_data_bytes": data_bytes,
           "sst_index_bytes": index_bytes}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
