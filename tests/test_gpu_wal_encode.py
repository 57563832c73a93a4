"""lsmck_wal_encode_batch on the GPU against the oracle's wal_insert /
wal_remove concatenation, byte for byte: the batches of wal_encode_cases.py
(whose coverage tests/test_wal_encode_cases.py proves on the CPU) at the
smallest shapes, every length and alignment, every tile edge, a realistic
mixed batch that replays, shared sources, offsets across 2^32, the guards
around the image, every error, the host form and CommandLog.log_batch."""
import io
import struct
import zlib

import numpy as np
import pytest

import wal_encode_cases as W
from lsm_storage_engine_amd import _lib, wal
from lsm_storage_engine_amd.device import WalEncodeError
from oracle import oracle as O

pytestmark = pytest.mark.gpu
AA = 0xAA


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.get_stat("wal_encode_tile")
    assert t in W.TILES  # a power of two, 256 .. 65536: what the case tests cover
    return t


_images = {}


def oracle_image(b):
    """A batch's oracle image, computed once."""
    if b.name not in _images:
        _images[b.name] = np.frombuffer(b.oracle_image(), dtype=np.uint8)
    return _images[b.name]


class DeviceBatch:
    """A batch's arenas and commands on the device, and an image buffer filled
    with 0xAA whose image base is `shift` bytes past a multiple of T, GUARD
    bytes of the buffer (and more) in front of it and `slack` behind cap."""

    def __init__(self, ctx, b, T, shift=0, cap=None, slack=64):
        self.ctx, self.b, self.n = ctx, b, len(b)
        self.total = b.rec_off()[1]
        self.cap = self.total if cap is None else cap
        self.bufs = []
        self.dk = self._up(b.keys)
        self.dv = self.dk if b.vals is b.keys else self._up(b.vals)
        self.dc = self._up(b.cmds)
        self.drec = self._alloc(8 * max(self.n, 1))
        self.slack = slack
        self.dimg = self._alloc(W.GUARD + 2 * T + self.cap + slack)
        ctx.memset(self.dimg.ptr, AA, self.dimg.nbytes)
        ctx.sync()
        self.img_ptr = (self.dimg.ptr + W.GUARD + T - 1) // T * T + shift
        self.img_off = self.img_ptr - self.dimg.ptr

    def _alloc(self, nbytes):
        d = self.ctx.alloc(max(nbytes, 1))
        self.bufs.append(d)
        return d

    def _up(self, a):
        d = self._alloc(a.nbytes)
        if a.nbytes:
            d.upload(a)
        return d

    def encode(self, cap=None):
        b = self.b
        return self.ctx.wal_encode_batch_device(self.dk.ptr, b.keys.nbytes, self.dv.ptr, b.vals.nbytes, self.dc.ptr,
                                                self.n, self.img_ptr, self.cap if cap is None else cap, self.drec.ptr)

    def whole(self):
        return self.dimg.download()

    def image(self, nbytes):
        return self.dimg.download(np.uint8, nbytes, self.img_off)

    def rec_off(self):
        return self.drec.download(np.uint64, self.n)

    def untouched_around(self, nbytes):
        """Everything of the buffer but image bytes [0, nbytes) is still 0xAA."""
        w = self.whole()
        return bool((w[:self.img_off] == AA).all() and (w[self.img_off + nbytes:] == AA).all())

    def free(self):
        for d in self.bufs:
            d.free()


def check(ctx, b, T, shift=0, extra_cap=0):
    """Encode on the device and compare: image, offsets, size, guards."""
    want = oracle_image(b)
    off, total = b.rec_off()
    assert len(want) == total
    d = DeviceBatch(ctx, b, T, shift, cap=total + extra_cap)
    try:
        got_bytes = d.encode()
        assert got_bytes == total
        img = d.image(total)
        if not np.array_equal(img, want):
            bad = np.nonzero(img != want)[0]
            r = np.searchsorted(off, bad[:6], side="right") - 1
            raise AssertionError(f"{b}: shift {shift}: {len(bad)} bytes differ, first at {bad[:6].tolist()} = records "
                                 f"{r.tolist()} + {(bad[:6] - off[r]).tolist()} (tile {T}: {(bad[:6] + shift) % T})")
        assert np.array_equal(d.rec_off(), off)
        assert d.untouched_around(total), f"{b}: shift {shift}: bytes outside the image were written"
    finally:
        d.free()


# --- smallest shapes ---------------------------------------------------------
@pytest.mark.parametrize("i", range(4))
def test_one_record(ctx, T, i):
    for shift in (0, 1, 3, 15):
        check(ctx, W.smallest()[i], T, shift)


def test_empty_removes_in_a_row(ctx, T):
    check(ctx, W.empty_removes(), T)


def test_first_and_last_payload_empty(ctx, T):
    check(ctx, W.empty_ends(), T)
    check(ctx, W.empty_ends(), T, shift=3)


def test_no_commands(ctx):
    img, off = ctx.wal_encode_batch(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, _lib.WAL_CMD_DTYPE))
    assert len(img) == 0 and len(off) == 0
    assert ctx.wal_encode_batch_device(0, 0, 0, 0, 0, 0, 0, 0) == 0
    with pytest.raises(_lib.LsmckError) as e:  # a flag bit the call does not know
        ctx._wal_encode(0, 0, 0, 0, 0, 0, 0, 0, None, _lib.DEVICE | 0x40)
    assert e.value.rc == _lib.EINVAL


# --- lengths and alignment ------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_lengths_and_alignments(ctx, T, shift):
    """Keys and values of 0..48 bytes at every source residue mod 16 and every
    destination residue, the image base at img + 0, 1, 3, 15."""
    check(ctx, W.lengths_alignment(), T, shift, extra_cap=100)


# --- tile edges --------------------------------------------------------------------
def test_tile_edges_in_insert_headers(ctx, T):
    check(ctx, W.tile_inserts(T), T)


def test_tile_edges_in_remove_headers(ctx, T):
    check(ctx, W.tile_removes(T), T)


def test_tile_edges_at_key_value_boundaries(ctx, T):
    check(ctx, W.tile_mix(T), T)


@pytest.mark.parametrize("plus", [0, 1])
def test_image_of_whole_tiles_and_one_byte_more(ctx, T, plus):
    check(ctx, W.tile_sized(T, 3, plus), T)
    check(ctx, W.tile_sized(T, 3, plus), T, shift=15)


# --- a realistic batch ----------------------------------------------------------------
def test_zipf_mixed_batch_replays(ctx, T):
    b = W.zipf_mixed()
    assert len(b) == 200_000
    want = oracle_image(b)
    off, total = b.rec_off()
    d = DeviceBatch(ctx, b, T)
    try:
        assert d.encode() == total
        assert np.array_equal(d.image(total), want)
        assert np.array_equal(d.rec_off(), off)
        recs, status, _ = ctx.wal_replay_verify(total, device_ptr=d.img_ptr)
        assert status == 0 and len(recs) == len(b)
        assert np.array_equal(recs["rec_off"], off)
        assert np.array_equal(recs["type"], b.cmds["type"])
    finally:
        d.free()


# --- shared and repeated sources ------------------------------------------------------
def test_keys_and_values_in_one_arena(ctx, T):
    b = W.shared_arena()
    assert b.vals is b.keys
    check(ctx, b, T)
    img, off = ctx.wal_encode_batch(b.keys, b.keys, b.cmds)  # host form: the arena uploaded once
    assert np.array_equal(img, oracle_image(b)) and np.array_equal(off, b.rec_off()[0])


def test_many_commands_one_value(ctx, T):
    check(ctx, W.one_value(), T, shift=1)


# --- offsets across 2^32 ------------------------------------------------------------------
def test_offsets_across_4gib(ctx, T):
    """70 Inserts of one 64 MiB value, then 1000 small records: the image is
    ~4.4 GiB and is checked where it is -- replay, offsets, every whole
    record's CRC-32 on the device against zlib's of the expected bytes -- and
    its small tail byte for byte."""
    keys, cmds = W.big_commands()
    n, nbig = len(cmds), 70
    value = O.gen_stream(W.BIG_SEED, 0, W.BIG_VALUE)
    b = W.Batch("big", keys, value[:2048], cmds)  # (sizes and the small records' sources)
    off, total = b.rec_off()
    sizes = b.sizes()
    assert total > 1 << 32
    bufs = [ctx.alloc(x) for x in (keys.nbytes, W.BIG_VALUE, cmds.nbytes, 8 * n, total, 4 * n, 4 * n)]
    dk, dv, dc, drec, dimg, dlen, dcrc = bufs
    try:
        dk.upload(keys)
        dc.upload(cmds)
        ctx.gen_stream(dv.ptr, W.BIG_SEED, 0, W.BIG_VALUE)
        ctx.sync()
        assert ctx.wal_encode_batch_device(dk.ptr, keys.nbytes, dv.ptr, W.BIG_VALUE, dc.ptr, n, dimg.ptr, total,
                                           drec.ptr) == total
        assert np.array_equal(drec.download(np.uint64, n), off)
        recs, status, _ = ctx.wal_replay_verify(total, device_ptr=dimg.ptr, cap=n)
        assert status == 0 and len(recs) == n and np.array_equal(recs["rec_off"], off)
        # expected CRC of every whole record
        cv = zlib.crc32(value)
        want = np.empty(n, dtype=np.uint32)
        for i in range(n):
            k, vl, vo = b.key(i).tobytes(), int(cmds["vlen"][i]), int(cmds["val_off"][i])
            if cmds["type"][i] == W.REMOVE:
                want[i] = zlib.crc32(struct.pack("<BII", 2, zlib.crc32(k), len(k)) + k)
            elif i < nbig:
                head = struct.pack("<BIII", 1, W.crc_concat(zlib.crc32(k), cv, vl), len(k), vl) + k
                want[i] = W.crc_concat(zlib.crc32(head), cv, vl)
            else:
                v = value[vo:vo + vl].tobytes()
                want[i] = zlib.crc32(struct.pack("<BIII", 1, zlib.crc32(k + v), len(k), vl) + k + v)
        dlen.upload(sizes.astype(np.uint32))
        ctx.crc32_device(dimg.ptr, drec.ptr, dlen.ptr, n, dcrc.ptr)
        ctx.sync()
        got = dcrc.download(np.uint32, n)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        # the small tail, byte for byte
        t0 = int(off[nbig])
        small = W.Batch("big_tail", keys, value[:2048], cmds[nbig:])
        assert np.array_equal(dimg.download(np.uint8, total - t0, t0), np.frombuffer(small.oracle_image(), np.uint8))
    finally:
        for d in bufs:
            d.free()


# --- guards -------------------------------------------------------------------------------------
def test_guards_before_and_behind_the_image(ctx, T):
    """64 bytes of 0xAA before img are unchanged, and so is img[total .. cap)."""
    b = W.lengths_alignment()
    total = b.rec_off()[1]
    for shift in (0, 7):
        d = DeviceBatch(ctx, b, T, shift, cap=total + 5000)
        try:
            assert d.encode() == total
            w = d.whole()
            assert (w[d.img_off - W.GUARD:d.img_off] == AA).all()
            assert (w[d.img_off + total:d.img_off + total + 5000] == AA).all()
            assert d.untouched_around(total)
            assert np.array_equal(d.image(total), oracle_image(b))
        finally:
            d.free()


# --- errors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_invalid_command_is_refused(ctx, T, case):
    name, b, idx, _ = W.invalid_cases()[case]
    d = DeviceBatch(ctx, b, T, cap=4096)
    try:
        with pytest.raises(WalEncodeError) as e:
            d.encode()
        assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx, name
        assert (d.whole() == AA).all(), f"{name}: the image buffer was written"
    finally:
        d.free()
    with pytest.raises(WalEncodeError) as e:  # the host form reports the same command
        ctx.wal_encode_batch(b.keys, b.vals, b.cmds)
    assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx


def test_wild_remove_value_is_accepted(ctx, T):
    check(ctx, W.wild_remove(), T)


def test_short_buffer_is_enospc(ctx, T):
    b = W.empty_ends()
    total = b.rec_off()[1]
    d = DeviceBatch(ctx, b, T, cap=total - 1, slack=64)
    try:
        with pytest.raises(WalEncodeError) as e:
            d.encode()
        assert e.value.rc == _lib.ENOSPC and e.value.needed == total and e.value.bad_index is None
        assert (d.whole() == AA).all()
        assert d.encode(cap=total) == total  # (the buffer holds `slack` more) and the context is fine afterwards
        assert np.array_equal(d.image(total), oracle_image(b))
    finally:
        d.free()


# --- host form and log_batch -------------------------------------------------------------------------
def test_host_form_equals_device_form(ctx, T):
    b = W.zipf_mixed(n=20_000)
    b.name = "zipf_20k"
    off, total = b.rec_off()
    d = DeviceBatch(ctx, b, T)
    try:
        assert d.encode() == total
        dev_img, dev_off = d.image(total), d.rec_off()
    finally:
        d.free()
    assert np.array_equal(dev_img, oracle_image(b))
    img, roff = ctx.wal_encode_batch(b.keys, b.vals, b.cmds)  # pageable
    assert np.array_equal(img, dev_img) and np.array_equal(roff, dev_off)
    pk, pv = ctx.alloc_pinned(b.keys.nbytes), ctx.alloc_pinned(b.vals.nbytes)
    try:
        pk.array[:], pv.array[:] = b.keys, b.vals
        img, roff = ctx.wal_encode_batch(pk.array, pv.array, b.cmds, pinned=True)
        assert np.array_equal(img, dev_img) and np.array_equal(roff, dev_off)
    finally:
        pk.free()
        pv.free()


def test_log_batch_leaves_the_file_log_leaves(ctx, tmp_path):
    recs = W.lengths_alignment().records()[:3000] + W.empty_ends().records()
    a, bb = wal.CommandLog(io.BytesIO()), wal.CommandLog(io.BytesIO())
    a.insert(b"before", b"the batch")  # (the batch is appended to what is there)
    bb.insert(b"before", b"the batch")
    want = [a.log(r) for r in recs]
    assert bb.log_batch(recs, ctx) == want
    assert bb.inner() == a.inner()
    # and on a file, through MemTable.from_log with and without the GPU
    path = tmp_path / "wal" / "log"
    f = wal.CommandLog.new(str(path))
    f.log_batch(recs, ctx)
    assert open(path, "rb").read() == a.inner()[len(O.wal_insert(b"before", b"the batch")):]
    cpu = wal.MemTable.from_log(wal.CommandLog.new(str(path)))
    gpu = wal.MemTable.from_log(wal.CommandLog.new(str(path)), ctx)
    assert list(gpu) == list(cpu) and gpu.size_in_bytes() == cpu.size_in_bytes() and cpu.size() > 0
