"""The stream kernel at its slice boundaries (crc32_stream_kernel and
stream_cut, lsmck_crc32.hip; the plan: lsmck_splan.h).  A batch of more than
64 records per wave is cut by the slice plan, and a wave goes from one slice
to the next it draws.
The cases sit where that can go wrong at a small size:
  * slices of one or two tiles (a tile is a slice's first and last), with
    neighbours sharing a 128-byte chunk, n a multiple of 64 and not;
  * the same with WAL-style gaps and short records (< 64 B, checksummed by
    their window lane) first and last in slices: a third of the records are
    short, and so are the records on both sides of every other cut of the
    plan (found from the plan and the offsets), the batch's first and last;
  * 150 records a wave with one 3 MiB record in the middle (empty slices, a
    wave handed an empty slice) and one as the batch's last record (a carry
    over many tiles into the tile clamped at the batch's end);
  * the record counts on both sides of the plan's first threshold (one slice
    per wave against one more), read from the plan itself.
Every batch: an unaligned base (ptr + 1), off[0] not chunk-aligned, the last
record ending on the allocation's last byte, the checked and the
caller-asserted entry, each launched twice in a row (the ticket counter is
reset by every launch), against oracle.crc32_batch (computed once a case)."""
import zlib

import numpy as np
import pytest

import splan_model
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NCU = 256
WAVES = 4096  # 256 CUs x 16
MIB = 1 << 20


def _offsets(lens, gaps):
    step = gaps.astype(np.uint64)
    step[1:] += lens[:-1].astype(np.uint64)
    return np.cumsum(step, dtype=np.uint64) + np.uint64(5)


def _lens(kind, n, rng):
    if kind == "packed":
        return rng.choice([64, 65, 100, 127, 128, 129, 200, 300], n), np.zeros(n, dtype=np.int64)
    if kind == "wal":  # 13- or 9-byte headers between the payloads, a third of them under 64 bytes
        lens = np.where(rng.random(n) < 0.33, rng.integers(1, 64, n), rng.integers(64, 300, n))
        gaps = rng.choice([13, 9], n)
        # Short records first and last in slices: at each cut record a of the
        # plan, record a is made short and its bytes given to a + 1, and
        # record a - 1 is made short and its bytes given to a - 2 where it
        # then still starts in front of the cut's byte target -- so off[a],
        # and with it the cut, stays.  (Cuts under four records apart are left.)
        lens[0] = 9
        lens[n - 1] = 7
        off = _offsets(lens, gaps)
        cut, target = splan_model.cuts(NCU, off, lens, targets=True)
        prev = 0
        for a, t in zip(cut[1:-1], target[1:]):
            a, t = int(a), int(t)
            if a < prev + 4 or a + 3 >= n:
                continue
            prev = a
            if lens[a] >= 64:
                short = int(rng.integers(1, 64))
                lens[a + 1] += lens[a] - short
                lens[a] = short
            need = int(off[a]) - int(gaps[a]) - t + 1  # a - 1 must keep its start under the target
            if lens[a - 1] >= 64 and need <= 63:
                short = int(rng.integers(max(1, need), 64))
                lens[a - 2] += lens[a - 1] - short
                lens[a - 1] = short
        return lens, gaps
    assert kind == "big"
    lens = rng.integers(40, 120, n)
    lens[n // 2] = 3 * MIB
    lens[n - 1] = 3 * MIB
    return lens, np.zeros(n, dtype=np.int64)


@pytest.mark.parametrize("n,kind", [(64 * WAVES + 64, "packed"), (64 * WAVES + 127, "packed"),
                                    (64 * WAVES + 64, "wal"), (64 * WAVES + 127, "wal"),
                                    (150 * WAVES + 17, "big"),
                                    ("first", "threshold"), ("below", "threshold")])
def test_handover_vs_oracle(ctx, n, kind):
    label = kind  # (the threshold cases draw their own batches)
    if kind == "threshold":  # the plan's first threshold, read from the plan (built when the test runs)
        n1 = splan_model.first_n_over_one_slice_per_wave(NCU)
        lib = splan_model.load()
        assert lib.splan_slices(NCU, n1) == WAVES + 1 and lib.splan_slices(NCU, n1 - 1) == WAVES
        n, kind = (n1 if n == "first" else n1 - 1), "packed"
    rng = np.random.default_rng(zlib.crc32(f"handover{n}{kind}{label}".encode()))
    lens, gaps = _lens(kind, n, rng)
    lens = lens.astype(np.uint32)
    off = _offsets(lens, gaps)
    if label == "wal":  # the generator's aim, checked: slices begin, and many end, with a short record
        cut = splan_model.cuts(NCU, off, lens)
        lo, hi = cut[:-1], cut[1:]
        full = hi > lo
        first_short = lens[np.minimum(lo, n - 1)] < 64
        last_short = lens[np.maximum(hi, 1) - 1] < 64
        assert (full & first_short).sum() >= 0.95 * full.sum()
        assert (full & first_short & last_short).sum() >= WAVES // 3
    nbytes = int(off[-1]) + int(lens[-1])  # the last record ends on the buffer's last byte
    assert nbytes + 1 < 64 * MIB
    data = O.gen_stream(0x4A0D0E00 + n % 251, 0, nbytes)
    want = O.crc32_batch(data, off, lens, threads=8)
    d = ctx.alloc(nbytes + 1)
    d_o, d_l, out = ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    try:
        d.upload(data, offset=1)
        d_o.upload(off)
        d_l.upload(lens)
        ctx.set_option("crc_stream", 2)  # the stream kernel alone
        try:
            for sorted_span in (False, False, True, True):
                out.upload(np.full(n, 0xA5A5A5A5, dtype=np.uint32))  # unwritten outputs show
                ctx.crc32_device(d.ptr + 1, d_o.ptr, d_l.ptr, n, out.ptr, sorted_span=sorted_span)
                ctx.sync()
                got = out.download(np.uint32)
                assert np.array_equal(got, want), (sorted_span, np.nonzero(got != want)[0][:8])
        finally:
            ctx.set_option("crc_stream", 1)
    finally:
        for b in (d, d_o, d_l, out):
            b.free()
