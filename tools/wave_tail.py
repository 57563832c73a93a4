#!/usr/bin/env python3
"""When the stream kernel's waves finish (crc32_stream_kernel, lsmck_crc32.hip).

A library built with the per-wave marks,
  EXTRA="-DLSMCK_WAVE_DIAG" tools/build_ab.sh wdiag WT
appends for every launch, to the file LSMCK_WAVE_DIAG_OUT names, a header
{magic, waves, records, 0} and per wave {clock at entry, clock at exit, event
tiles << 32 | tiles without events, HW_ID | XCC_ID << 32} (u64 each; the clock
is the constant 100 MHz one, 10 ns a tick).  This script reports per launch:
  * the kernel's span (first entry to last exit) and the spread of the entries;
  * the span from the first wave's finish to the last wave's finish, over the
    chip and per workgroup (= per CU: one 1024-thread workgroup each);
  * the wave-time lost to the tail: mean over the waves of (last exit - exit);
  * the least-squares fit  wave time = a + b * tiles + c * event tiles, and
    c / b (an event tile's extra cost in tiles without events).

  python3 tools/wave_tail.py wave_diag.bin [--json out.json] [--min-records N]
"""
import json
import sys

import numpy as np

MAGIC = 0x4741494445564157
TICK_US = 0.01


def launches(path):
    a = np.fromfile(path, dtype=np.uint64)
    i = 0
    while i + 4 <= len(a):
        if int(a[i]) != MAGIC:
            raise SystemExit(f"bad header at u64 {i}")
        nw, nrec = int(a[i + 1]), int(a[i + 2])
        yield nrec, a[i + 4:i + 4 + 4 * nw].reshape(nw, 4)
        i += 4 + 4 * nw


def report(nrec, w):
    t0, t1 = w[:, 0].astype(np.int64), w[:, 1].astype(np.int64)
    ev, no = (w[:, 2] >> np.uint64(32)).astype(np.int64), (w[:, 2] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    busy = (ev + no) > 0
    if busy.sum() < 8:
        return None
    t0, t1, ev, no = t0[busy], t1[busy], ev[busy], no[busy]
    cu = np.nonzero(busy)[0] // 16
    begin, end = t0.min(), t1.max()
    span = (end - begin) * TICK_US
    dur = (t1 - t0) * TICK_US
    per_cu = np.array([(t1[cu == c].max() - t1[cu == c].min()) * TICK_US for c in np.unique(cu)])
    cu_end = np.array([(t1[cu == c].max() - begin) * TICK_US for c in np.unique(cu)])
    A = np.stack([np.ones(len(dur)), (ev + no).astype(float), ev.astype(float)], axis=1)
    coef, *_ = np.linalg.lstsq(A, dur, rcond=None)
    resid = dur - A @ coef
    r = {
        "records": nrec, "waves": int(busy.sum()), "kernel_span_us": round(span, 1),
        "entry_spread_us": round((t0.max() - t0.min()) * TICK_US, 1),
        "finish_first_to_last_us": round((t1.max() - t1.min()) * TICK_US, 1),
        "finish_p50_to_last_us": round((t1.max() - np.median(t1)) * TICK_US, 1),
        "finish_p95_to_last_us": round((t1.max() - np.percentile(t1, 95)) * TICK_US, 1),
        "tail_loss_frac_of_span": round(float(np.mean(end - t1)) * TICK_US / span, 4),
        "per_cu_finish_span_us": {"median": round(float(np.median(per_cu)), 1), "max": round(float(per_cu.max()), 1)},
        "cu_last_exit_spread_us": round(float(cu_end.max() - cu_end.min()), 1),
        "tiles_per_wave": {"mean": round(float((ev + no).mean()), 1), "sd": round(float((ev + no).std()), 2)},
        "event_tiles_per_wave": {"mean": round(float(ev.mean()), 1), "sd": round(float(ev.std()), 2)},
        "wave_time_us": {"mean": round(float(dur.mean()), 1), "sd": round(float(dur.std()), 2)},
        "fit_us": {"const": round(float(coef[0]), 2), "per_tile": round(float(coef[1]), 4),
                   "per_event_tile_extra": round(float(coef[2]), 4), "resid_sd": round(float(resid.std()), 2)},
        "event_tile_extra_in_tiles": round(float(coef[2] / coef[1]), 3) if coef[1] else None,
    }
    return r


def main():
    path = sys.argv[1]
    min_rec = int(sys.argv[sys.argv.index("--min-records") + 1]) if "--min-records" in sys.argv else 0
    out = [r for nrec, w in launches(path) if nrec >= min_rec for r in [report(nrec, w)] if r]
    for k, r in enumerate(out):
        print(f"launch {k}: " + json.dumps(r))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
