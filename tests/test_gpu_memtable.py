"""lsmck_memtable_build and lsmck_wal_recs_to_cmds on the GPU against the cases
module's expected values (memtable_cases.py: wal.MemTable.from_log over the
log's records, whose meaning tests/test_memtable_cases.py proves on the CPU),
entry for entry: the entries as (key bytes, value bytes) through the arenas,
src, nent, mem_bytes and the round count; the outputs between 0xAA guards that
must stay intact, as must everything past nent.  Then the adapter from the
replay's compact records, MemTable.from_image and sstable.flush_log_image
against the host path's files."""
import filecmp
import os
import struct
import zlib

import numpy as np
import pytest

import memtable_cases as M
from lsm_storage_engine_amd import _lib, sstable, wal
from lsm_storage_engine_amd.device import MemBuildError, WAL_REC16_DTYPE, decode_rec16

pytestmark = pytest.mark.gpu
AA = 0xAA
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class DeviceLog:
    """A log's arenas (each allocated at exactly its size) and commands on
    the device, and the two outputs -- ents and src of `cap` entries -- each
    between GUARD bytes of 0xAA and filled with 0xAA."""

    def __init__(self, ctx, g, cap=None, base=0):
        self.ctx, self.g, self.n = ctx, g, len(g)
        self.cap = self.n + 3 if cap is None else cap
        self.bufs = []
        self.dk = self._up(g.keys)
        self.dv = self.dk if g.vals is g.keys else self._up(g.vals)
        self.dc = self._up(g.cmds)
        self.dents = self._filled(2 * M.GUARD + 32 * self.cap)
        self.dsrc = self._filled(2 * M.GUARD + 4 * self.cap)
        ctx.sync()

    def _alloc(self, nbytes):
        d = self.ctx.alloc(max(nbytes, 1))
        self.bufs.append(d)
        return d

    def _filled(self, nbytes):
        d = self._alloc(nbytes)
        self.ctx.memset(d.ptr, AA, d.nbytes)
        return d

    def _up(self, a):
        d = self._alloc(a.nbytes)
        if a.nbytes:
            d.upload(a)
        return d

    def build(self, cap=None, src=True):
        g = self.g
        return self.ctx.memtable_build_device(self.dk.ptr, g.keys.nbytes, self.dv.ptr, g.vals.nbytes, self.dc.ptr, self.n,
                                              self.dents.ptr + M.GUARD, self.cap if cap is None else cap,
                                              self.dsrc.ptr + M.GUARD if src else None)

    def outputs(self, nent):
        """(ents[:nent], src[:nent]) and whether every other byte of both buffers is still 0xAA."""
        e, s = self.dents.download(), self.dsrc.download()
        g = M.GUARD
        ok = (e[:g] == AA).all() and (e[g + 32 * nent:] == AA).all() and (s[:g] == AA).all() and \
            (s[g + 4 * nent:] == AA).all()
        return e[g:g + 32 * nent].view(_lib.WAL_CMD_DTYPE), s[g:g + 4 * nent].view(np.uint32), bool(ok)

    def free(self):
        for d in self.bufs:
            d.free()


def through_arenas(g, ents):
    kb, vb = g.keys.tobytes(), g.vals.tobytes()
    return [(kb[ko:ko + kl], vb[vo:vo + vl]) for ko, kl, vo, vl in
            zip(ents["key_off"].tolist(), ents["klen"].tolist(), ents["val_off"].tolist(), ents["vlen"].tolist())]


def check_log(ctx, g, cap=None):
    entries, nbytes, src, rounds = g.expected()
    d = DeviceLog(ctx, g, cap)
    try:
        got = d.build()
        print(g.name, "nent, mem_bytes:", got, "rounds:", ctx.get_stat("mem_rounds"), "expected:", len(entries), nbytes,
              rounds)
        assert got == (len(entries), nbytes)
        assert ctx.get_stat("mem_rounds") == rounds
        ents, s, guards = d.outputs(got[0])
        assert guards
        assert (ents["type"] == 1).all() and (ents["reserved"] == 0).all()
        assert s.tolist() == src
        assert through_arenas(g, ents) == entries
        return ents.copy(), s.copy()
    finally:
        d.free()


LOGS = M.smallest() + M.order() + M.round_counts()[:5] + M.residues() + M.stability() + M.active_edges() + M.shared()


@pytest.mark.parametrize("g", LOGS, ids=lambda g: g.name)
def test_log(ctx, g):
    check_log(ctx, g)


@pytest.mark.parametrize("n", M.SIZES)
def test_sizes(ctx, n):
    check_log(ctx, M.sized(n), cap=n)


def test_big_twice(ctx):
    """2^18 commands over 2^12 distinct keys of 0..24 bytes from {0, 1, 0xFF}, run twice with identical output."""
    g = M.big()
    a = check_log(ctx, g)
    b = check_log(ctx, g)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_without_src_and_exact_cap(ctx):
    g = M.stability()[3]
    entries, nbytes, _, _ = g.expected()
    d = DeviceLog(ctx, g, cap=len(entries))
    try:
        assert d.build(src=False) == (len(entries), nbytes)
        ents, _, _ = d.outputs(len(entries))
        assert through_arenas(g, ents) == entries
        assert (d.dsrc.download() == AA).all()
        e = d.dents.download()
        assert (e[:M.GUARD] == AA).all() and (e[M.GUARD + 32 * len(entries):] == AA).all()
    finally:
        d.free()


def test_ranges_around_4gib(ctx):
    """keys == vals: one arena just above 4 GiB, every range inside the 8 KiB
    around offset 2^32, keys and values that straddle it included."""
    base, span = (1 << 32) - 4096, 8192
    rng = np.random.default_rng(41)
    piece = rng.integers(0, 3, span, dtype=np.uint8)
    n = 2000
    c = np.zeros(n, dtype=_lib.WAL_CMD_DTYPE)
    c["type"] = np.where(rng.integers(0, 6, n) == 0, M.REMOVE, M.INSERT)
    c["klen"], c["vlen"] = rng.integers(0, 20, n), rng.integers(0, 20, n)
    c["key_off"], c["val_off"] = rng.integers(4096 - 40, 4096 + 40, n), rng.integers(4096 - 40, 4096 + 40, n)
    c["key_off"][:4], c["klen"][:4] = [4096 - 3, 4096 - 8, 4096, 4095], [9, 8, 9, 1]  # across, up to, from, the last byte below
    g = M.Log("around_4gib", piece, piece, c)
    entries, nbytes, src, rounds = g.expected()
    arena_bytes = (1 << 32) + 4096
    arena, dc, dents, dsrc = bufs = [ctx.alloc(arena_bytes), ctx.alloc(c.nbytes), ctx.alloc(32 * n), ctx.alloc(4 * n)]
    try:
        arena.upload(piece, offset=base)
        dev = c.copy()
        dev["key_off"] += np.uint64(base)
        dev["val_off"] += np.uint64(base)
        dc.upload(dev)
        got = ctx.memtable_build_device(arena.ptr, arena_bytes, arena.ptr, arena_bytes, dc.ptr, n, dents.ptr, n, dsrc.ptr)
        assert got == (len(entries), nbytes) and ctx.get_stat("mem_rounds") == rounds
        ents = dents.download(_lib.WAL_CMD_DTYPE, got[0])
        assert (ents["key_off"] >= base).all() and (ents["key_off"] + ents["klen"] > 1 << 32).any()
        ents["key_off"] -= np.uint64(base)
        ents["val_off"] -= np.uint64(base)
        assert through_arenas(g, ents) == entries and dsrc.download(np.uint32, got[0]).tolist() == src
    finally:
        for d in bufs:
            d.free()


# --- errors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.invalid_cases(), ids=lambda c: c[0])
def test_invalid_command(ctx, case):
    name, g, idx = case
    d = DeviceLog(ctx, g)
    try:
        with pytest.raises(MemBuildError) as e:
            d.build()
        assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx and e.value.needed is None
        assert d.outputs(0)[2]
    finally:
        d.free()


def test_enospc(ctx):
    g = M.sized(1023)
    entries, nbytes, _, _ = g.expected()
    d = DeviceLog(ctx, g)
    try:
        for cap in (len(entries) - 1, 0):
            with pytest.raises(MemBuildError) as e:
                d.build(cap=cap)
            assert e.value.rc == _lib.ENOSPC and e.value.needed == len(entries) and e.value.bad_index is None
            assert d.outputs(0)[2]
    finally:
        d.free()


def test_enospc_sets_mem_bytes(ctx):
    import ctypes as C
    g = M.sized(257)
    entries, nbytes, _, _ = g.expected()
    d = DeviceLog(ctx, g)
    try:
        nent, nb, bad = C.c_size_t(), C.c_uint64(), C.c_uint64()
        rc = ctx.lib.lsmck_memtable_build(ctx.handle, d.dk.ptr, g.keys.nbytes, d.dv.ptr, g.vals.nbytes, d.dc.ptr, len(g),
                                          d.dents.ptr + M.GUARD, 1, d.dsrc.ptr + M.GUARD, C.byref(nent), C.byref(nb),
                                          C.byref(bad), _lib.DEVICE)
        assert (rc, nent.value, nb.value, bad.value) == (_lib.ENOSPC, len(entries), nbytes, 2 ** 64 - 1)
        assert d.outputs(0)[2]
    finally:
        d.free()


# --- the host form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [M.sized(4097), M.shared()[0], M.shared()[1], M.smallest()[0], M.order()[3]],
                         ids=lambda g: g.name)
def test_host_form_equals_the_device_form(ctx, g):
    """The arenas as two arrays and (shared_arena, overlapping_ranges) as one."""
    entries, nbytes, src, rounds = g.expected()
    dev_ents, dev_src = check_log(ctx, g)
    for pinned in (False, True):
        ents, s, nb = ctx.memtable_build(g.keys, g.vals, g.cmds, pinned=pinned)
        assert nb == nbytes and ctx.get_stat("mem_rounds") == rounds
        assert ents.tobytes() == dev_ents.tobytes() and s.tolist() == dev_src.tolist() == src
        assert through_arenas(g, ents) == entries
    name, bad, idx = M.invalid_cases()[4]
    with pytest.raises(MemBuildError) as e:
        ctx.memtable_build(bad.keys, bad.vals, bad.cmds)
    assert e.value.bad_index == idx


# --- the adapter --------------------------------------------------------------------------------------
def insert_record(klen, vlen, data):
    """An Insert record whose header names klen / vlen over `data`, the payload actually there (its CRC refit)."""
    return struct.pack("<BIII", 1, zlib.crc32(data), klen, vlen) + data


def mixed_log(n, seed, keys=300):
    rng = np.random.default_rng(seed)
    log = wal.CommandLog.new_in_memory()
    for i in range(n):
        k = b"key-%d" % int(rng.integers(0, keys))
        if rng.integers(0, 5) == 0:
            log.remove(k)
        else:
            log.insert(k, rng.bytes(int(rng.integers(0, 40))))
    return log.inner()


def to_cmds(ctx, image):
    """The image's replay with compact records on the device, converted: (commands, status)."""
    img = np.frombuffer(image, np.uint8)
    cap = len(img) // 9 + 1
    dimg, drecs = ctx.alloc(max(len(img), 1)), ctx.alloc(16 * cap)
    try:
        dimg.upload(img)
        nrec, status, _ = ctx.wal_replay_verify_to_device(len(img), drecs.ptr, cap, device_ptr=dimg.ptr, compact=True)
        dcmds = ctx.alloc(32 * max(nrec, 1) + 2 * M.GUARD)
        try:
            ctx.memset(dcmds.ptr, AA, dcmds.nbytes)
            ctx.wal_recs_to_cmds_device(drecs.ptr, nrec, len(img), dcmds.ptr + M.GUARD)
            ctx.sync()
            w = dcmds.download()
            assert (w[:M.GUARD] == AA).all() and (w[M.GUARD + 32 * nrec:] == AA).all()
            return w[M.GUARD:M.GUARD + 32 * nrec].view(_lib.WAL_CMD_DTYPE).copy(), \
                drecs.download(WAL_REC16_DTYPE, nrec), status
        finally:
            dcmds.free()
    finally:
        dimg.free()
        drecs.free()


def build_over_image(ctx, image, cmds):
    img = np.frombuffer(image, np.uint8)
    return ctx.memtable_build(img, img, cmds)


def test_adapter_against_decode_rec16(ctx):
    image = mixed_log(3000, 5)
    cmds, recs, status = to_cmds(ctx, image)
    assert status == 0 and len(cmds) == 3000
    r = decode_rec16(recs)
    assert (cmds["key_off"] == r["payload_off"]).all() and (cmds["klen"] == r["klen"]).all()
    assert (cmds["val_off"] == r["payload_off"] + r["klen"].astype(np.uint64)).all()
    assert (cmds["vlen"] == r["vlen"]).all() and (cmds["type"] == r["type"]).all() and (cmds["reserved"] == 0).all()
    want = wal.MemTable.from_log(wal.CommandLog.new_in_memory(image))
    ents, _, nbytes = build_over_image(ctx, image, cmds)
    g = M.Log("image", np.frombuffer(image, np.uint8), np.frombuffer(image, np.uint8), cmds)
    assert through_arenas(g, ents) == sorted(want.data.items()) and nbytes == want.bytes


def test_adapter_last_insert_cut_inside_its_value(ctx):
    """The header names 30 value bytes, 11 are there and the CRC covers them: accepted with the shorter value."""
    image = mixed_log(50, 6) + insert_record(4, 30, b"keyA" + b"short value")
    want = wal.MemTable.from_log(wal.CommandLog.new_in_memory(image))
    assert want.data[b"keyA"] == b"short value"
    cmds, _, status = to_cmds(ctx, image)
    assert status == 0 and len(cmds) == 51
    assert (int(cmds["klen"][-1]), int(cmds["vlen"][-1])) == (4, 11)
    assert int(cmds["val_off"][-1]) + 11 == len(image)
    got = wal.MemTable.from_image(image, ctx)
    assert got.data == want.data and got.bytes == want.bytes


@pytest.mark.parametrize("kind", ["cut_inside_key", "wrapped_sum", "wrapped_then_more"])
def test_adapter_key_past_the_payload_is_einval(ctx, kind):
    head = mixed_log(40, 7)
    if kind == "cut_inside_key":  # 10 key bytes named, 6 there
        image = head + insert_record(10, 5, b"sixbyt")
    else:  # klen + vlen wraps to 16 in u32
        image = head + insert_record(0xFFFFFFF0, 0x20, b"0123456789abcdef")
        if kind == "wrapped_then_more":
            image += mixed_log(10, 8)
    with pytest.raises(wal.WalPanic) as want:
        wal.MemTable.from_log(wal.CommandLog.new_in_memory(image))
    cmds, _, status = to_cmds(ctx, image)
    assert status == 0 and len(cmds) == (51 if kind == "wrapped_then_more" else 41)
    with pytest.raises(MemBuildError) as e:
        build_over_image(ctx, image, cmds)
    assert e.value.rc == _lib.EINVAL and e.value.bad_index == 40
    with pytest.raises(wal.WalPanic) as got:
        wal.MemTable.from_image(image, ctx)
    assert str(got.value) == str(want.value)


def test_from_image_raises_the_replays_errors(ctx):
    for kind, exc in (("insert", wal.CorruptedData), ("remove", wal.WalPanic), ("type", wal.InvalidCommandType)):
        one = wal.CommandLog.new_in_memory()
        one.insert(b"kk", b"vvvv") if kind == "insert" else one.remove(b"kkkk")
        rec = bytearray(one.inner())
        rec[0 if kind == "type" else -1] ^= 0x55  # the type byte, or the payload's last byte
        image = mixed_log(100, 9) + bytes(rec) + mixed_log(10, 12)
        with pytest.raises(exc) as a:
            wal.MemTable.from_log(wal.CommandLog.new_in_memory(image))
        with pytest.raises(exc) as b:
            wal.MemTable.from_image(image, ctx)
        assert str(a.value) == str(b.value)


# --- the pipeline ----------------------------------------------------------------------------------------
def test_from_image_equals_from_log(ctx):
    for image in (open(os.path.join(GOLDEN, "wal_2000.bin"), "rb").read(), mixed_log(20_000, 10, keys=3000), b""):
        want = wal.MemTable.from_log(wal.CommandLog.new_in_memory(image))
        got = wal.MemTable.from_image(image, ctx)
        assert got.data == want.data and got.bytes == want.bytes


def test_flush_log_image_writes_the_host_paths_files(ctx, tmp_path):
    image = mixed_log(20_000, 11, keys=3000)
    a, b = tmp_path / "gpu", tmp_path / "host"
    m = sstable.flush_log_image(str(a), image, ctx, timestamp_ms=1700000000123)
    want = sstable.from_memtable(str(b), wal.MemTable.from_log(wal.CommandLog.new_in_memory(image)), ctx=None,
                                 timestamp_ms=1700000000123)
    assert os.path.getsize(want.data_path()) > 40_000
    for x, y in ((m.data_path(), want.data_path()), (m.index_path(), want.index_path()),
                 (m.checksum_path(), want.checksum_path())):
        assert filecmp.cmp(x, y, shallow=False), x
    rep = ctx.tree_verify(str(a))
    assert rep["tables"] == 1 and rep["bad_tables"] == 0


def test_flush_log_image_every_key_removed(ctx, tmp_path):
    log = wal.CommandLog.new_in_memory()
    for i in range(300):
        log.insert(b"k%d" % (i % 100), b"v%d" % i)
    for i in range(100):
        log.remove(b"k%d" % i)
    a, b = tmp_path / "gpu", tmp_path / "host"
    m = sstable.flush_log_image(str(a), log.inner(), ctx, timestamp_ms=5)
    want = sstable.from_memtable(str(b), wal.MemTable.from_log(wal.CommandLog.new_in_memory(log.inner())), ctx=None,
                                 timestamp_ms=5)
    assert os.path.getsize(m.data_path()) == 0 and open(m.index_path(), "rb").read() == b"\0" * 8
    for x, y in ((m.data_path(), want.data_path()), (m.index_path(), want.index_path()),
                 (m.checksum_path(), want.checksum_path())):
        assert filecmp.cmp(x, y, shallow=False), x
    assert ctx.tree_verify(str(a))["bad_tables"] == 0
