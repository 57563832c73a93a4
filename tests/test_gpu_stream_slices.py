"""The stream kernel's slices (crc32_stream_kernel, lsmck_crc32.hip): a batch of
more than 64 records per wave is cut into up to 16 slices per wave, which the
waves take one after the other from a ticket counter.  Which wave checksums a
record is then decided at run time; the CRCs must not depend on it.

Sizes: 4096 waves on the MI355X, so the slices outnumber the waves from
2^18 + 64 records on and reach 16 per wave at 2^22 records.  The batches here
sit just under and just over the first threshold (one slice per wave, no
ticket taken, against 4097 slices) and in between, with records short enough
that each batch stays under 64 MiB; the full 16 slices per wave run in
test_gpu_crc.py's full-size config-3 digests.  Every batch is checked against
oracle.crc32_batch, through the checked and the caller-asserted entry, and
twice over: the ticket counter is reset by every launch."""
import zlib

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

WAVES = 4096  # 256 CUs x 16


def _device(ctx, d, off, ln, sorted_span):
    n = len(off)
    d_o, d_l, out = ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    out.upload(np.full(n, 0xA5A5A5A5, dtype=np.uint32))  # unwritten outputs show
    d_o.upload(off)
    d_l.upload(ln)
    ctx.set_option("crc_stream", 2)  # the stream kernel alone
    try:
        ctx.crc32_device(d.ptr + 1, d_o.ptr, d_l.ptr, n, out.ptr, sorted_span=sorted_span)
        ctx.sync()
    finally:
        ctx.set_option("crc_stream", 1)
    got = out.download(np.uint32)
    for b in (d_o, d_l, out):
        b.free()
    return got


@pytest.mark.parametrize("n,kind", [(64 * WAVES + 63, "packed"), (64 * WAVES + 64, "packed"),
                                    (64 * WAVES + 64, "wal"), (150 * WAVES + 17, "zipf")])
def test_slices_vs_oracle(ctx, n, kind):
    rng = np.random.default_rng(zlib.crc32(f"{n}{kind}".encode()))
    if kind == "packed":
        lens = rng.choice([64, 65, 100, 127, 128, 129, 200, 300], n)
        gaps = np.zeros(n, dtype=np.int64)
    elif kind == "wal":  # 13- or 9-byte headers between the payloads, a third of them under 64 bytes
        lens = np.where(rng.random(n) < 0.3, rng.integers(1, 64, n), rng.integers(64, 300, n))
        gaps = rng.choice([13, 9], n)
    else:
        from lsm_storage_engine_amd.device import gen_zipf_lengths
        lens = np.minimum(gen_zipf_lengths(78, n), 200)  # (capped: the batch stays small)
        gaps = np.zeros(n, dtype=np.int64)
        lens[n // 2] = 3 << 20  # one record over many slices' worth of bytes: its neighbours' slices are empty
    lens = lens.astype(np.uint32)
    step = gaps.astype(np.uint64)
    step[1:] += lens[:-1]
    off = np.cumsum(step, dtype=np.uint64) + np.uint64(5)
    data = O.gen_stream(0x57AE0F00 + n % 251, 0, int(off[-1]) + int(lens[-1]) + 16)
    want = O.crc32_batch(data, off, lens, threads=8)
    d = ctx.alloc(len(data) + 1)
    d.upload(data, offset=1)
    try:
        for sorted_span in (False, True, False):
            got = _device(ctx, d, off, lens, sorted_span)
            assert np.array_equal(got, want), (sorted_span, np.nonzero(got != want)[0][:8])
    finally:
        d.free()
