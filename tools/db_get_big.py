#!/usr/bin/env python3
"""Full-size batch Db::get on the GPU: lsmck_db_get_batch, device form.

tools/get_big.py's first shape -- 4 tables of 2^22 entries written on the
device by lsmck_sstable_encode_batch (setup, not timed), table t holding the
keys 8i + t, and 2^20 uniform queries, half present -- with two runs in front:
run 0 of 2^18 and run 1 of 2^20 entries.  A quarter of the queries' keys are put
into the runs (a fifth of them into run 0), the rest of the runs' entries are
keys nobody asks for, so about a quarter of the queries hit a run.  Every stage
is timed between device events ("sst_encode_time"): the run pass, the index
pass, the run probe, the table probe, resolve + scan, the gather; the counters
give the pairs looked up, the pairs walked and the run hits.  Yardsticks in the
same process: lsmck_sstable_get_batch over the same tables and queries, a
device-to-device hipMemcpyAsync of the gathered bytes, and a torch.searchsorted
of 2^20 int64 probes into 2^20 sorted int64 keys (the run probe's).  The
results are checked: the sources against the construction, the gathered bytes
of a sample of queries against their sources.  Writes one JSON line (--out)
and prints it.

  python3 tools/db_get_big.py [--log2 22] [--reps 3] [--out profiles/r12/dbget/db_get_big.json]
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
from get_big import key_bytes, searchsorted_ms  # noqa: E402  (tools/get_big.py, beside this file)

DB = ("runs", "index", "run_probe", "probe", "resolve", "gather")
GET = ("index", "probe", "resolve")
GIB = float(1 << 30)


def device_run(ctx, lo, kmax, seed):
    """A run over the sorted u64 keys `lo` (16-byte keys, Zipf value lengths): (descriptor tuple, buffers, vlen, val_off)."""
    n = len(lo)
    vlen = gen_zipf_lengths(seed, n, kmax=kmax).astype(np.uint64) - np.uint64(16)
    ents = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    ents["type"], ents["klen"], ents["vlen"] = 1, 16, vlen
    ents["key_off"] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    ents["val_off"] = np.cumsum(vlen) - vlen
    vb = int(vlen.sum())
    dk, dv, de = ctx.alloc(16 * n), ctx.alloc(max(vb, 1)), ctx.alloc(ents.nbytes)
    dk.upload(key_bytes(np.zeros(n, dtype=np.uint64), lo).ravel())
    ctx.gen_stream(dv.ptr, seed ^ 0xA5, 0, vb)
    de.upload(ents)
    return (dk.ptr, 16 * n, dv.ptr, vb, de.ptr, n), (dk, dv, de), vlen, ents["val_off"].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=22, help="entries per table")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--run0", type=int, default=1 << 18)
    ap.add_argument("--run1", type=int, default=1 << 20)
    ap.add_argument("--kmax", type=int, default=64, help="Zipf lengths on k = 1..kmax (L = 64k - j)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=512, help="queries whose gathered bytes are compared with their source")
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "dbget", "db_get_big.json"))
    a = ap.parse_args()
    ctx = Context(0)
    ntab, m, nq = 4, 1 << a.log2, a.queries
    n = ntab * m
    rng = np.random.default_rng(0x6E7)
    # the tables: get_big's shape `one`
    vlen = gen_zipf_lengths(0x5EED0003, n, kmax=a.kmax).astype(np.uint64) - np.uint64(16)
    i = np.tile(np.arange(m, dtype=np.uint64), ntab)
    t = np.repeat(np.arange(ntab, dtype=np.uint64), m)
    lo = np.uint64(8) * i + t
    ents = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    ents["type"], ents["klen"], ents["vlen"] = 1, 16, vlen
    ents["key_off"] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    ents["val_off"] = np.cumsum(vlen) - vlen
    first = np.arange(ntab + 1, dtype=np.uint64) * np.uint64(m)
    kb, vb = 16 * n, int(vlen.sum())
    db, ib = n * 24 + vb, ntab * 8 + ntab * ((m + 99) // 100) * 32
    dk, dv, de = ctx.alloc(kb), ctx.alloc(max(vb, 1)), ctx.alloc(ents.nbytes)
    dk.upload(key_bytes(np.zeros(n, dtype=np.uint64), lo).ravel())
    ctx.gen_stream(dv.ptr, 0x5EED00A2, 0, vb)
    de.upload(ents)
    ddata, dindex, dspans = ctx.alloc(db), ctx.alloc(ib), ctx.alloc(32 * ntab)
    assert ctx.sstable_encode_batch_device(dk.ptr, kb, dv.ptr, vb, de.ptr, n, first, ddata.ptr, db, dindex.ptr, ib,
                                           dspans.ptr) == (db, ib)
    for b in (dk, dv, de):
        b.free()
    # the queries: even ones present (a uniform entry), odd ones absent (a uniform gap)
    pick = rng.integers(0, n, nq)
    qlo = lo[pick].copy()
    absent = np.arange(nq) % 2 == 1
    qlo[absent] = (qlo[absent] & ~np.uint64(7)) + np.uint64(4) + (pick[absent].astype(np.uint64) & np.uint64(3))
    # the runs: a quarter of the queries' distinct keys, a fifth of them in run 0; the rest keys nobody asks for
    # (8i + 4..7 gaps with bit 63 set lie above every table key and every query)
    asked = np.unique(qlo[rng.random(nq) < 0.25])
    to0 = rng.random(len(asked)) < 0.2
    filler = np.uint64(1 << 63) + np.arange(a.run0 + a.run1, dtype=np.uint64) * np.uint64(3)
    r0 = np.sort(np.concatenate([asked[to0], filler[:max(a.run0 - int(to0.sum()), 0)]]))
    r1 = np.sort(np.concatenate([asked[~to0], filler[a.run0:a.run0 + max(a.run1 - int((~to0).sum()), 0)]]))
    runs, bufs, rvlen, rvoff = [], [], [], []
    for r, keys in enumerate((r0, r1)):
        desc, bb, vl, vo = device_run(ctx, keys, a.kmax, 0x5EED0100 + r)
        runs.append(desc), bufs.append(bb), rvlen.append(vl), rvoff.append(vo)
    qkeys = key_bytes(np.zeros(nq, dtype=np.uint64), qlo).ravel()
    q = np.zeros(nq, dtype=_lib.GET_QUERY_DTYPE)
    q["klen"], q["key_off"] = 16, np.arange(nq, dtype=np.uint64) * np.uint64(16)
    dqk, dq, dres, doff = ctx.alloc(qkeys.nbytes), ctx.alloc(q.nbytes), ctx.alloc(16 * nq), ctx.alloc(8 * (nq + 1))
    dqk.upload(qkeys)
    dq.upload(q)
    # what the construction says: the source and the answered length of every query
    in0, in1 = np.isin(qlo, r0), np.isin(qlo, r1)
    src = np.where(in0, 0, np.where(in1, 1, np.where(absent, _lib.GET_NONE, 2 + t[pick]))).astype(np.uint32)
    alen = np.where(in0, rvlen[0][np.searchsorted(r0, qlo) % len(r0)],
                    np.where(in1, rvlen[1][np.searchsorted(r1, qlo) % len(r1)], np.where(absent, np.uint64(0), vlen[pick]))).astype(np.uint64)
    total = int(alen.sum())
    dout = ctx.alloc(max(total, 1))
    args = (dqk.ptr, qkeys.nbytes, dq.ptr, nq, dres.ptr)
    tabs = (ddata.ptr, db, dindex.ptr, ib, dspans.ptr, ntab)
    out = {"metric": "batch Db::get on the device (stage times between device events)", "kmax": a.kmax, "reps": a.reps,
           "tables": ntab, "entries_per_table": m, "run_entries": [len(r0), len(r1)], "queries": nq,
           "data_bytes": db, "run_value_bytes": [runs[0][3], runs[1][3]]}
    ctx.set_option("sst_encode_time", 1)
    whole, stages = [], {s: [] for s in DB}
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        got = ctx.db_get_batch_device(runs, *tabs, *args, dout.ptr, total, doff.ptr)
        dt = (time.perf_counter() - t0) * 1e3
        ms = {s: ctx.get_stat(f"db_get_{s}_ns") / 1e6 for s in DB}
        cnt = {k: ctx.get_stat(f"db_get_{k}") for k in ("probed", "walked", "run_hits")}
        print(f"db get {r}: {dt:.2f} ms, stages {ms}, {cnt}", file=sys.stderr, flush=True)
        assert got == total
        if r:
            whole.append(dt)
            for s in DB:
                stages[s].append(ms[s])
    out["db_get_ms"] = round(float(np.median(whole)), 3)
    out["db_get_stage_ms"] = {s: round(float(np.median(v)), 3) for s, v in stages.items()}
    out["db_get_stage_ms_all"] = {s: [round(x, 3) for x in v] for s, v in stages.items()}
    out["pairs_probed"], out["pairs_walked"], out["run_hits"] = cnt["probed"], cnt["walked"], cnt["run_hits"]
    out["run_hit_share"] = round(cnt["run_hits"] / nq, 4)
    out["bytes_gathered"] = total
    out["gather_gib_s"] = round(total / GIB / (out["db_get_stage_ms"]["gather"] / 1e3), 1)
    res = dres.download(_lib.GET_RESULT_DTYPE, nq)
    off = doff.download(np.uint64, nq + 1)
    assert np.array_equal(res["table"], src), "every query's source is the construction's"
    assert np.array_equal(np.diff(off), alen) and cnt["run_hits"] == int((src < 2).sum())
    spans = dspans.download(_lib.SSTABLE_SPAN_DTYPE, ntab)
    for j in rng.choice(np.nonzero(alen)[0], a.sample, replace=False).tolist():
        s, vo, vl = int(res["table"][j]), int(res["val_off"][j]), int(res["vlen"][j])
        want = (bufs[s][1] if s < 2 else ddata).download(np.uint8, vl, vo)
        assert np.array_equal(dout.download(np.uint8, vl, int(off[j])), want), j
    assert spans["data_len"].sum() == db
    # yardstick 1: lsmck_sstable_get_batch over the same tables and queries
    get_stages = {s: [] for s in GET}
    for r in range(a.reps + 1):
        ctx.sstable_get_batch_device(*tabs, *args)
        if r:
            for s in GET:
                get_stages[s].append(ctx.get_stat(f"sst_get_{s}_ns") / 1e6)
    out["sstable_get_stage_ms"] = {s: round(float(np.median(v)), 3) for s, v in get_stages.items()}
    out["sstable_get_pairs_probed"] = ctx.get_stat("sst_get_probed")
    out["sstable_get_pairs_walked"] = ctx.get_stat("sst_get_walked")
    out["table_probe_over_sstable_get_probe"] = round(out["db_get_stage_ms"]["probe"] /
                                                      out["sstable_get_stage_ms"]["probe"], 3)
    ctx.set_option("sst_encode_time", 0)
    # yardstick 2: hipMemcpyAsync device to device, the gathered byte count
    a_, b_ = (torch.empty(total, dtype=torch.uint8, device="cuda") for _ in range(2))
    a_.fill_(0x5A)
    ts = []
    for r in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b_.copy_(a_)  # same dtype, contiguous: hipMemcpyAsync(hipMemcpyDeviceToDevice)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    out["copy_d2d_ms"] = round(float(np.median(ts)), 3)
    out["gather_share_of_copy"] = round(out["copy_d2d_ms"] / out["db_get_stage_ms"]["gather"], 3)
    # yardstick 3: a searchsorted of 2^20 int64 probes into 2^20 sorted int64 keys, for the run probe
    out["searchsorted_ms"] = searchsorted_ms(1 << 20, 1 << 20, a.reps)
    out["run_probe_over_searchsorted"] = round(out["db_get_stage_ms"]["run_probe"] / out["searchsorted_ms"], 2)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
