"""The stream kernel's event tiles (crc32_stream_kernel, lsmck_crc32.hip): a
record boundary at every byte position of a 128-byte chunk, for every kind of
boundary a chunk can hold -- an end alone, a start alone, an end and a start
at the same byte (packed records), an end and the next start 1, 13 or 64 bytes
later, two ends in one chunk (64-byte records, one per chain), records under
64 bytes between long ones.  The per-word event bodies run under the EXEC
mask on the lanes that hold the event; these batches put an event in every
word of both chains, in chunks 0 and 63 of a tile and on a tile edge.

Every batch is three tiles (24 KiB) long, runs with the base pointer at byte
offsets 0..3, through the checked entry and the caller-asserted one
(LSMCK_SORTED), and is checked against oracle.crc32_batch.  (The 32-bit
record window was measured slower and is not in the tree, DESIGN.md 3.1, so
there is no crc_win switch to run both ways.)  In a batch this small every
record is a slice of its own (the cuts are balanced by bytes), so one more
batch joins all of them, repeated to 63 MiB: there a slice holds some sixty
consecutive records, a wave meets both events of a boundary, and the waves
take several slices each."""
import numpy as np
import pytest

from oracle import oracle as O

TILE = 8192
SPAN = 3 * TILE
SEED = 0x57AE0E00


def _records(kind, lead):
    """(off, len, wide_gaps) of one batch; wide_gaps: gaps over 64 bytes (LSMCK_SORTED only)"""
    off, ln = [], []
    if kind in ("packed", "gap1", "gap13", "gap64"):
        g = 0 if kind == "packed" else int(kind[3:])
        k = 0
        while lead + 129 * (k + 1) <= SPAN:  # boundary k at byte lead + 129 k: chunk k (+1 past 128), position k mod 128
            off.append(lead + 129 * k + g)
            ln.append(129 - g)
            k += 1
    elif kind == "ends_starts":  # odd chunks hold a start alone, even chunks an end alone (lead: the position's phase)
        j = 0
        while 128 * (2 * j + 3) <= SPAN:
            p = (j + lead) % 128
            off.append(128 * (2 * j + 1) + p)
            ln.append(128)
            j += 1
    elif kind == "two_ends":  # 64- and 65-byte records: two boundaries per chunk, one per chain
        o = lead
        while o + 65 <= SPAN:
            l = 64 + (len(off) & 1)
            off.append(o)
            ln.append(l)
            o += l
    elif kind == "shorts":  # a record of 1..63 bytes between two long ones
        k = 0
        while lead + 129 * (k + 1) <= SPAN:
            s = 1 + (2 * k) % 63
            off += [lead + 129 * k, lead + 129 * (k + 1) - s]
            ln += [129 - s, s]
            k += 1
    else:
        raise ValueError(kind)
    return np.asarray(off, dtype=np.uint64), np.asarray(ln, dtype=np.uint32), kind == "ends_starts"


BATCHES = [(k, lead) for k in ("packed", "gap1", "gap13", "gap64", "two_ends", "shorts") for lead in (0, 65)] + \
          [("ends_starts", 0), ("ends_starts", 64)]
IDS = [f"{k}-{lead}" for k, lead in BATCHES]


def _events(off, ln):
    """(ends, starts) of the long records: positions relative to the chunk grid's origin"""
    a0 = int(off[0]) & ~127
    lng = ln >= 64
    return (off[lng] + ln[lng]).astype(np.int64) - a0, off[lng].astype(np.int64) - a0


def test_batches_cover_the_event_positions():
    """(no GPU) what the batches are built to hold, with the base pointer at offset 0"""
    allb = []
    for kind in ("packed", "gap1", "gap13", "gap64", "two_ends", "shorts", "ends_starts"):
        ends, starts = [], []
        for k, lead in BATCHES:
            if k != kind:
                continue
            off, ln, _ = _records(k, lead)
            assert int(off[-1]) + int(ln[-1]) <= SPAN and int(off[-1]) + int(ln[-1]) > 2 * TILE  # three tiles
            e, s = _events(off, ln)
            ends.append(e)
            starts.append(s)
            if kind == "ends_starts":  # a chunk holds one event
                ch = np.concatenate([e >> 7, s >> 7])
                assert len(np.unique(ch)) == len(ch)
            if kind == "two_ends":  # two ends per chunk, one per chain
                c, cnt = np.unique(e >> 7, return_counts=True)
                two = c[cnt == 2]  # (all but the few chunks where the pair's second end moves on a chunk)
                assert len(two) > 180 and {0, 63} & set((two & 63).tolist())
                assert all(sorted(((e[(e >> 7) == x] >> 6) & 1).tolist()) == [0, 1] for x in two)
            if kind.startswith("gap"):  # the end and the next start in the same chunk, wherever they fit
                g = int(kind[3:])
                same = ((e[:-1] >> 7) == (s[1:] >> 7))
                assert (same == ((e[:-1] & 127) + g < 128)).all() and same.any()
            if kind == "shorts":
                assert ((ln < 64).sum() * 2 == len(ln)) and set(ln[ln < 64].tolist()) == set(range(1, 64))
        ends, starts = np.concatenate(ends), np.concatenate(starts)
        assert set((ends & 127).tolist()) == set(range(128)), kind   # an end at every byte of a chunk
        assert set((starts & 127).tolist()) == set(range(128)), kind  # and a start
        allb += [ends, starts]
    b = np.concatenate(allb)
    assert {0, 15, 16, 31} <= set(((b & 127) >> 2).tolist())  # words 0 and 15 of both chains
    assert {0, 63} <= set(((b >> 7) & 63).tolist())           # the first and the last chunk of a tile
    assert (b[b > 0] % TILE == 0).any()                        # a boundary on a tile edge


def _device(ctx, data, off, ln, shift, sorted_span):
    n = len(off)
    d = ctx.alloc(len(data) + shift)
    d.upload(data, offset=shift)
    d_o, d_l, out = ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(4 * n)
    out.upload(np.full(n, 0xA5A5A5A5, dtype=np.uint32))  # unwritten outputs show
    d_o.upload(off)
    d_l.upload(ln)
    ctx.crc32_device(d.ptr + shift, d_o.ptr, d_l.ptr, n, out.ptr, sorted_span=sorted_span)
    ctx.sync()
    got = out.download(np.uint32)
    for b in (d, d_o, d_l, out):
        b.free()
    return got


def _run(ctx, data, off, ln, shift, sorted_span):
    """the stream kernel alone (a declined batch would leave the outputs unwritten)"""
    ctx.set_option("crc_stream", 2)
    try:
        return _device(ctx, data, off, ln, shift, sorted_span)
    finally:
        ctx.set_option("crc_stream", 1)


@pytest.fixture(scope="module")
def stream():
    return O.gen_stream(SEED, 0, SPAN + 64)


_want = {}


def _oracle(stream, kind, lead):
    if (kind, lead) not in _want:
        off, ln, wide = _records(kind, lead)
        _want[(kind, lead)] = (off, ln, wide, O.crc32_batch(stream, off, ln))
    return _want[(kind, lead)]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,lead", BATCHES, ids=IDS)
def test_event_positions(ctx, stream, kind, lead, shift):
    off, ln, wide, want = _oracle(stream, kind, lead)
    if not wide:  # (gaps over 64 bytes: the device check declines the batch)
        got = _run(ctx, stream, off, ln, shift, False)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    srt = _run(ctx, stream, off, ln, shift, True)
    assert np.array_equal(srt, want), np.nonzero(srt != want)[0][:8]


@pytest.mark.gpu
def test_event_positions_many_records_per_wave(ctx):
    """All the batches above one after the other, 192 times, each copy 1..61
    bytes after the one before (every alignment of every pattern): 63 MiB, so
    that a slice holds some sixty consecutive records and the waves take
    several slices each."""
    offs, lns = [], []
    base = 0
    for rep in range(192):
        for kind, lead in BATCHES:
            off, ln, _ = _records(kind, lead)
            offs.append(off - off[0] + np.uint64(base))
            lns.append(ln)
            base = int(offs[-1][-1]) + int(ln[-1]) + 1 + rep % 61
    off, ln = np.concatenate(offs), np.concatenate(lns)
    data = O.gen_stream(SEED + 1, 0, base + 64)
    want = O.crc32_batch(data, off, ln, threads=8)
    assert len(off) > 64 * 4096 * 2  # more slices than waves
    got = _run(ctx, data, off, ln, 3, True)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
