#!/usr/bin/env python3
"""Full-size gets over an opened table set: lsmck_tableset_open and
lsmck_tableset_get_batch, device form, beside lsmck_db_get_batch (nrun = 0) on
the same inputs in the same process.

tools/get_big.py's two shapes, built the same way (the tables written on the
device by lsmck_sstable_encode_batch, 2^20 queries, half present):
  many  --order tables of 1,024 entries asked as ONE search order; a group of 4
        tables shares a key range, the groups are disjoint, so the fences drop
        every pair outside a query's group;
  one   4 tables of 2^22 entries that interleave: the fences prune almost
        nothing, and the probe pays the fence test on every pair.
One warm-up and --reps repetitions, the two calls alternating.  Stage times are
between device events ("sst_encode_time"), which also makes both probes count
their pairs.  For each shape the JSON holds the yardstick's stages with their
spread (max - min over the repetitions), the set's open and get stages, the
pairs fenced / looked up / walked, and the two comparisons:
  many  set probe  <  yardstick index + probe - yardstick spread   ("beats")
  one   set probe  <= yardstick probe + yardstick spread           ("no_worse")
The results of the two calls are compared byte for byte.

--bloom-bits B (4..64) adds, per shape, a second set opened with "bloom_bits" B
beside the one opened with 0: the open's stages with the filters' own
("tableset_open_bloom_ns"), then the two sets' gets alternating in the same
process -- probe and resolve times, the pairs fenced / bloomed / looked up /
walked of each -- and the two results compared byte for byte ("bloom" in the
JSON).

  python3 tools/tableset_big.py [--log2 22] [--order 256] [--reps 3] [--bloom-bits 12]
                                [--out profiles/r14/tableset/tableset_big.json]
"""
import argparse
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
from tools.get_big import key_bytes  # noqa: E402

YARD = ("index", "probe", "resolve")
SET = ("probe", "resolve")


def med(v):
    return round(float(np.median(v)), 3)


def spread(v):
    return round(float(max(v) - min(v)), 3)


def bloom_part(ctx, name, ts, reps, bits, open_args, get_args, dres, dres3, nq, ntab):
    """The set opened with ``bits`` per key beside ``ts`` (opened with 0): open stages, alternating gets, counts."""
    ctx.set_option("sst_encode_time", 1)
    ctx.set_option("bloom_bits", bits)
    opens, stage = [], {"index": [], "fence": [], "bloom": []}
    tb = None
    try:
        for r in range(reps + 1):
            if tb is not None:
                tb.close()
            t0 = time.perf_counter()
            tb = ctx.tableset_open(*open_args[0], **open_args[1])
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                opens.append(dt)
                for s in stage:
                    stage[s].append(ctx.get_stat(f"tableset_open_{s}_ns") / 1e6)
    finally:
        ctx.set_option("bloom_bits", 0)
    out = {"bits": bits, "open_ms": med(opens), "open_spread_ms": spread(opens),
           "open_stage_ms": {s: med(v) for s, v in stage.items()},
           "set": {k: tb.stat(k) for k in ("bloom_tables", "bloom_keys", "bloom_bytes", "resident_bytes")}}
    names = ("fenced", "bloomed", "probed", "walked")
    times = {0: {s: [] for s in SET}, bits: {s: [] for s in SET}}
    whole, counts = {0: [], bits: []}, {}
    for r in range(reps + 1):
        for b, s_, d_ in ((0, ts, dres), (bits, tb, dres3)):
            t0 = time.perf_counter()
            s_.get_batch_device(*get_args, d_.ptr)
            dt = (time.perf_counter() - t0) * 1e3
            st = {s: ctx.get_stat(f"tableset_{s}_ns") / 1e6 for s in SET}
            counts[b] = {k: ctx.get_stat("tableset_" + k) for k in names}
            print(f"{name} bloom {r}: bits {b}: set get {dt:.2f} ms {st} {counts[b]}", file=sys.stderr, flush=True)
            if r:
                whole[b].append(dt)
                for s in SET:
                    times[b][s].append(st[s])
    ctx.set_option("sst_encode_time", 0)
    plain = {0: [], bits: []}  # untimed: no events, no pair counters
    for r in range(reps + 1):
        for b, s_, d_ in ((0, ts, dres), (bits, tb, dres3)):
            t0 = time.perf_counter()
            s_.get_batch_device(*get_args, d_.ptr)
            if r:
                plain[b].append((time.perf_counter() - t0) * 1e3)
    a, c = dres.download(_lib.GET_RESULT_DTYPE, nq), dres3.download(_lib.GET_RESULT_DTYPE, nq)
    assert a.tobytes() == c.tobytes(), "the set with filters answers as the set without"
    out["results_identical"] = True
    for b, key in ((0, "without"), (bits, "with")):
        out[key] = {"get_ms": med(whole[b]), "stage_ms": {s: med(v) for s, v in times[b].items()},
                    "stage_spread_ms": {s: spread(v) for s, v in times[b].items()}, "pairs": counts[b],
                    "uncounted_wall_ms": med(plain[b]), "uncounted_wall_spread_ms": spread(plain[b])}
    p0, p1 = out["without"]["stage_ms"]["probe"], out["with"]["stage_ms"]["probe"]
    out["probe_without_over_with"] = round(p0 / p1, 3) if p1 else None
    out["bloomed_share_of_unfenced"] = round(counts[bits]["bloomed"] / max(1, nq * ntab - counts[bits]["fenced"]), 4)
    tb.close()
    return out


def shape(ctx, name, ntab, m, nq, kmax, reps, bloom_bits=0):
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
    pick = rng.integers(0, n, nq)
    qhi, qlo = hi[pick].copy(), lo[pick].copy()
    absent = np.arange(nq) % 2 == 1
    qlo[absent] = (qlo[absent] & ~np.uint64(7)) + np.uint64(4) + (pick[absent].astype(np.uint64) & np.uint64(3)) \
        if name == "one" else qlo[absent] + np.uint64(1)
    qkeys = key_bytes(qhi, qlo).ravel()
    q = np.zeros(nq, dtype=_lib.GET_QUERY_DTYPE)
    q["klen"], q["key_off"] = 16, np.arange(nq, dtype=np.uint64) * np.uint64(16)
    dqk, dq, dres, dres2 = ctx.alloc(qkeys.nbytes), ctx.alloc(q.nbytes), ctx.alloc(16 * nq), ctx.alloc(16 * nq)
    dqk.upload(qkeys)
    dq.upload(q)
    ctx.set_option("sst_encode_time", 1)
    # the open: once per repetition too, so its time has a spread of its own
    opens, open_stage = [], {"index": [], "fence": []}
    ts = None
    for r in range(reps + 1):
        if ts is not None:
            ts.close()
        t0 = time.perf_counter()
        ts = ctx.tableset_open(ddata.ptr, dindex.ptr, dspans.ptr, ntab=ntab, data_bytes=db, index_bytes=ib)
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            opens.append(dt)
            open_stage["index"].append(ctx.get_stat("tableset_open_index_ns") / 1e6)
            open_stage["fence"].append(ctx.get_stat("tableset_open_fence_ns") / 1e6)
    out["open_ms"] = med(opens)
    out["open_stage_ms"] = {s: med(v) for s, v in open_stage.items()}
    out["set"] = {k: ts.stat(k) for k in ("tables", "items", "fenced_low", "fenced_high", "resident_bytes")}
    yard, mine = {s: [] for s in YARD}, {s: [] for s in SET}
    ywhole, swhole, counts, ycounts = [], [], {}, {}
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ctx.db_get_batch_device([], ddata.ptr, db, dindex.ptr, ib, dspans.ptr, ntab, dqk.ptr, qkeys.nbytes, dq.ptr, nq,
                                dres.ptr)
        yd = (time.perf_counter() - t0) * 1e3
        ys = {s: ctx.get_stat(f"db_get_{s}_ns") / 1e6 for s in YARD}
        ycounts = {k: ctx.get_stat("db_get_" + k) for k in ("probed", "walked")}
        t0 = time.perf_counter()
        ts.get_batch_device([], dqk.ptr, qkeys.nbytes, dq.ptr, nq, dres2.ptr)
        sd = (time.perf_counter() - t0) * 1e3
        ss = {s: ctx.get_stat(f"tableset_{s}_ns") / 1e6 for s in SET}
        counts = {k: ctx.get_stat("tableset_" + k) for k in ("fenced", "probed", "walked")}
        print(f"{name} {r}: db_get {yd:.2f} ms {ys} {ycounts}; set get {sd:.2f} ms {ss} {counts}", file=sys.stderr,
              flush=True)
        if r:
            ywhole.append(yd)
            swhole.append(sd)
            for s in YARD:
                yard[s].append(ys[s])
            for s in SET:
                mine[s].append(ss[s])
    ctx.set_option("sst_encode_time", 0)
    # the same calls untimed: no events and, above all, no pair counters in the probes (wall clock, synchronous calls)
    yplain, splain = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ctx.db_get_batch_device([], ddata.ptr, db, dindex.ptr, ib, dspans.ptr, ntab, dqk.ptr, qkeys.nbytes, dq.ptr, nq,
                                dres.ptr)
        t1 = time.perf_counter()
        ts.get_batch_device([], dqk.ptr, qkeys.nbytes, dq.ptr, nq, dres2.ptr)
        t2 = time.perf_counter()
        if r:
            yplain.append((t1 - t0) * 1e3)
            splain.append((t2 - t1) * 1e3)
    out["uncounted_wall_ms"] = {"db_get": med(yplain), "db_get_spread": spread(yplain), "set_get": med(splain),
                                "set_get_spread": spread(splain),
                                "db_get_over_set_get": round(med(yplain) / med(splain), 2)}
    a, b = dres.download(_lib.GET_RESULT_DTYPE, nq), dres2.download(_lib.GET_RESULT_DTYPE, nq)
    assert a.tobytes() == b.tobytes(), "the set's results are lsmck_db_get_batch's"
    assert np.array_equal(a["table"] != _lib.GET_NONE, ~absent), "every present key is found, no absent one"
    yip = [x + y for x, y in zip(yard["index"], yard["probe"])]
    out["db_get_ms"], out["db_get_stage_ms"] = med(ywhole), {s: med(v) for s, v in yard.items()}
    out["db_get_stage_spread_ms"] = {s: spread(v) for s, v in yard.items()}
    out["db_get_index_plus_probe_ms"], out["db_get_index_plus_probe_spread_ms"] = med(yip), spread(yip)
    out["db_get_pairs"] = ycounts
    out["set_get_ms"], out["set_get_stage_ms"] = med(swhole), {s: med(v) for s, v in mine.items()}
    out["set_get_stage_spread_ms"] = {s: spread(v) for s, v in mine.items()}
    out["set_pairs"] = counts
    out["fenced_share"] = round(counts["fenced"] / (nq * ntab), 4)
    p = out["set_get_stage_ms"]["probe"]
    out["index_plus_probe_over_set_probe"] = round(med(yip) / p, 2) if p else None
    out["probe_over_set_probe"] = round(out["db_get_stage_ms"]["probe"] / p, 3) if p else None
    out["beats_index_plus_probe_by_more_than_spread"] = bool(p < med(yip) - spread(yip))
    out["no_worse_than_probe_within_spread"] = bool(p <= out["db_get_stage_ms"]["probe"] + spread(yard["probe"]))
    out["fence_test_ns_per_pair"] = round((p - out["db_get_stage_ms"]["probe"]) * 1e6 / (nq * ntab), 4)
    if bloom_bits:
        out["bloom"] = bloom_part(ctx, name, ts, reps, bloom_bits,
                                  ((ddata.ptr, dindex.ptr, dspans.ptr), dict(ntab=ntab, data_bytes=db, index_bytes=ib)),
                                  ([], dqk.ptr, qkeys.nbytes, dq.ptr, nq), dres2, dres, nq, ntab)
    ts.close()
    for buf in (ddata, dindex, dspans, dqk, dq, dres, dres2):
        buf.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=22, help="shape `one`: entries per table")
    ap.add_argument("--order", type=int, default=256, help="shape `many`: tables of 1,024 entries in one search order")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--kmax", type=int, default=64, help="Zipf lengths on k = 1..kmax (L = 64k - j)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bloom-bits", type=int, default=0, help="also a set opened with this many filter bits per key (4..64)")
    ap.add_argument("--out", default=os.path.join("profiles", "r14", "tableset", "tableset_big.json"))
    a = ap.parse_args()
    ctx = Context(0)
    out = {"metric": "gets over an opened table set beside lsmck_db_get_batch (stage times between device events)",
           "kmax": a.kmax, "reps": a.reps,
           "many": shape(ctx, "many", a.order, 1024, a.queries, a.kmax, a.reps, a.bloom_bits),
           "one": shape(ctx, "one", 4, 1 << a.log2, a.queries, a.kmax, a.reps, a.bloom_bits)}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    ctx.close()


if __name__ == "__main__":
    main()
