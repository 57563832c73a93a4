#!/usr/bin/env python3
"""Full-size batch point reads on the GPU: lsmck_sstable_get_batch, device form.

tools/merge_big.py's two table layouts (Zipf value lengths capped by --kmax,
16-byte keys), the tables written on the device by lsmck_sstable_encode_batch
(setup, not timed) and queried where they lie:
  one   4 tables of 2^22 entries; table t holds the keys 8i + t, so a present
        key lies in one table and an absent one (8i + 4..7) between two keys
        of every table;
  many  tables of 1,024 entries in groups of 4 (merge_big's 4,096 groups' worth
        is --groups 4096); --order tables of them are asked as ONE search
        order (the tool states the size: every query is a work item against
        every table of the order); group g's table t holds the keys
        (g, 2 * (2i + bit t of i)), absent ones are odd.
2^20 queries (--queries), half present, drawn uniformly.  Every stage is timed
between device events ("sst_encode_time"): the index pass, the queries' check
plus the probe of every (query, table) pair, resolve; the probe's counters give
the share of pairs that were looked up (not skipped behind a lower table's
answer) and the share whose interval was walked.  Yardsticks in the same
process: the decode's segment-walk stage over the same tables (one walk of
every interval), lsmck_sstable_get on this thread over a sample of the queries
against one table (it parses the index on every call), and a torch.searchsorted
of as many int64 probes into as many sorted int64 keys as the tables hold.
Writes one JSON line (--out) and prints it.

  python3 tools/get_big.py [--log2 22] [--order 256] [--reps 3] [--out profiles/r11/get/get_big.json]
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
import torch  # noqa: E402  (before the library: the torch wheel's HIP runtime)
from lsm_storage_engine_amd import _lib  # noqa: E402
from lsm_storage_engine_amd.device import Context, gen_zipf_lengths  # noqa: E402

GET = ("index", "probe", "resolve")


def key_bytes(hi, lo):
    """16-byte keys: two big-endian u64."""
    n = len(lo)
    k = np.empty((n, 16), dtype=np.uint8)
    k[:, :8] = np.asarray(hi, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    k[:, 8:] = np.asarray(lo, dtype=np.uint64).astype(">u8").view(np.uint8).reshape(n, 8)
    return k


def searchsorted_ms(nkeys, nprobes, reps):
    keys = torch.arange(nkeys, dtype=torch.int64, device="cuda") * 8
    probes = torch.randint(0, 8 * nkeys, (nprobes,), dtype=torch.int64, device="cuda")
    ts = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.searchsorted(keys, probes)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))
    return round(float(np.median(ts)), 3)


def shape(ctx, name, ntab, m, nq, kmax, reps, sample):
    n = ntab * m
    rng = np.random.default_rng(0x6E7)
    ln = gen_zipf_lengths(0x5EED0003, n, kmax=kmax).astype(np.uint64)
    vlen = ln - np.uint64(16)
    i = np.tile(np.arange(m, dtype=np.uint64), ntab)
    t = np.repeat(np.arange(ntab, dtype=np.uint64), m)
    if name == "one":
        hi, lo = np.zeros(n, dtype=np.uint64), np.uint64(8) * i + t
    else:
        hi, lo = t >> np.uint64(2), np.uint64(2) * (np.uint64(2) * i + ((i >> (t & np.uint64(3))) & np.uint64(1)))
    keys = key_bytes(hi, lo).ravel()
    ents = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    ents["type"], ents["klen"], ents["vlen"] = 1, 16, vlen
    ents["key_off"] = np.arange(n, dtype=np.uint64) * np.uint64(16)
    ents["val_off"] = np.cumsum(vlen) - vlen
    first = np.arange(ntab + 1, dtype=np.uint64) * np.uint64(m)
    kb, vb = 16 * n, int(vlen.sum())
    db, ib = n * 24 + vb, ntab * 8 + ntab * ((m + 99) // 100) * 32
    dk, dv, de = ctx.alloc(kb), ctx.alloc(max(vb, 1)), ctx.alloc(ents.nbytes)
    dk.upload(keys)
    ctx.gen_stream(dv.ptr, 0x5EED00A2, 0, vb)
    de.upload(ents)
    ddata, dindex, dspans = ctx.alloc(db), ctx.alloc(ib), ctx.alloc(32 * ntab)
    assert ctx.sstable_encode_batch_device(dk.ptr, kb, dv.ptr, vb, de.ptr, n, first, ddata.ptr, db, dindex.ptr, ib,
                                           dspans.ptr) == (db, ib)
    for b in (dk, dv, de):
        b.free()
    out = {"shape": name, "tables": ntab, "entries_per_table": m, "queries": nq, "pairs": nq * ntab, "data_bytes": db,
           "index_bytes": ib}
    # the queries: even ones present (a uniform entry), odd ones absent (a uniform gap)
    pick = rng.integers(0, n, nq)
    qhi, qlo = hi[pick].copy(), lo[pick].copy()
    absent = np.arange(nq) % 2 == 1
    qlo[absent] = (qlo[absent] & ~np.uint64(7)) + np.uint64(4) + (pick[absent].astype(np.uint64) & np.uint64(3)) \
        if name == "one" else qlo[absent] + np.uint64(1)
    qkeys = key_bytes(qhi, qlo).ravel()
    q = np.zeros(nq, dtype=_lib.GET_QUERY_DTYPE)
    q["klen"], q["key_off"] = 16, np.arange(nq, dtype=np.uint64) * np.uint64(16)
    dqk, dq, dres = ctx.alloc(qkeys.nbytes), ctx.alloc(q.nbytes), ctx.alloc(16 * nq)
    dqk.upload(qkeys)
    dq.upload(q)
    ctx.set_option("sst_encode_time", 1)
    whole, stages, probed, walked = [], {s: [] for s in GET}, 0, 0
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ctx.sstable_get_batch_device(ddata.ptr, db, dindex.ptr, ib, dspans.ptr, ntab, dqk.ptr, qkeys.nbytes, dq.ptr, nq,
                                     dres.ptr)
        dt = (time.perf_counter() - t0) * 1e3
        ms = {s: ctx.get_stat(f"sst_get_{s}_ns") / 1e6 for s in GET}
        probed, walked = ctx.get_stat("sst_get_probed"), ctx.get_stat("sst_get_walked")
        print(f"get {name} {r}: {dt:.2f} ms, stages {ms}, probed {probed}, walked {walked}", file=sys.stderr, flush=True)
        if r:
            whole.append(dt)
            for s in GET:
                stages[s].append(ms[s])
    out["get_ms"] = round(float(np.median(whole)), 3)
    out["get_stage_ms"] = {s: round(float(np.median(v)), 3) for s, v in stages.items()}
    out["pairs_probed_share"] = round(probed / (nq * ntab), 4)  # (of the last repetition: the skips depend on timing)
    out["pairs_walked_share"] = round(walked / (nq * ntab), 4)
    out["probe_ns_per_query"] = round(out["get_stage_ms"]["probe"] * 1e6 / nq, 2)
    res = dres.download(_lib.GET_RESULT_DTYPE, nq)
    found = res["table"] != _lib.GET_NONE
    assert np.array_equal(found, ~absent), "every present key is found, no absent one"
    rt, pt = res["table"][found].astype(np.uint64), t[pick][found]
    if name == "one":
        assert np.array_equal(rt, pt), "in its table"
        assert np.array_equal(res["vlen"][found].astype(np.uint64), vlen[pick][found])
    else:  # (a key may lie in several tables of its group: the first of them answers)
        assert (rt <= pt).all() and np.array_equal(rt >> np.uint64(2), pt >> np.uint64(2)), "in its group"
    # yardstick 1: the decode's segment walk over the same tables -- one walk of every interval
    dents = ctx.alloc(32 * n)
    seg = []
    for r in range(reps + 1):
        ctx.sstable_decode_batch_device(ddata.ptr, db, dindex.ptr, ib, dspans.ptr, ntab, dents.ptr, n)
        if r:
            seg.append(ctx.get_stat("sst_decode_seg_ns") / 1e6)
    assert ctx.get_stat("sst_decode_declined") == 0
    out["decode_seg_walk_ms"] = round(float(np.median(seg)), 3)
    out["intervals"] = ntab * ((m + 99) // 100)
    dents.free()
    ctx.set_option("sst_encode_time", 0)
    # yardstick 2: the scalar call on this thread, one table, a sample of its present keys and of absent ones
    spans = dspans.download(_lib.SSTABLE_SPAN_DTYPE, ntab)
    s0 = spans[0]
    d0 = ddata.download(np.uint8, int(s0["data_len"]), int(s0["data_off"]))
    x0 = dindex.download(np.uint8, int(s0["index_len"]), int(s0["index_off"]))
    mine = np.nonzero((t[pick] == 0))[0][:sample]
    lib, off, vl = _lib.load(), C.c_uint64(), C.c_uint32()
    t0 = time.perf_counter()
    hits = 0
    for j in mine.tolist():
        hits += lib.lsmck_sstable_get(d0.ctypes.data, d0.nbytes, x0.ctypes.data, x0.nbytes, qkeys.ctypes.data + 16 * j, 16,
                                      C.byref(off), C.byref(vl))
    out["scalar_get_us_per_query"] = round((time.perf_counter() - t0) * 1e6 / max(len(mine), 1), 2)
    out["scalar_get_sample"] = len(mine)
    out["scalar_get_index_items"] = (m + 99) // 100
    assert hits == int((~absent[mine]).sum())
    # yardstick 3: a searchsorted of as many int64 probes into as many sorted int64 keys
    out["searchsorted_ms"] = searchsorted_ms(n, nq, reps)
    out["probe_over_searchsorted"] = round(out["get_stage_ms"]["probe"] / out["searchsorted_ms"], 2)
    out["probe_over_decode_seg_walk"] = round(out["get_stage_ms"]["probe"] / out["decode_seg_walk_ms"], 2)
    for b in (ddata, dindex, dspans, dqk, dq, dres):
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=22, help="shape `one`: entries per table")
    ap.add_argument("--order", type=int, default=256, help="shape `many`: tables of 1,024 entries in one search order")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--kmax", type=int, default=64, help="Zipf lengths on k = 1..kmax (L = 64k - j)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=256, help="queries of the scalar yardstick")
    ap.add_argument("--out", default=os.path.join("profiles", "r11", "get", "get_big.json"))
    a = ap.parse_args()
    ctx = Context(0)
    out = {"metric": "batch point reads on the device (stage times between device events)", "kmax": a.kmax,
           "reps": a.reps,
           "one": shape(ctx, "one", 4, 1 << a.log2, a.queries, a.kmax, a.reps, a.sample),
           "many": shape(ctx, "many", a.order, 1024, a.queries, a.kmax, a.reps, a.sample)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
