"""lsmck_sstable_encode_batch on the GPU against the cases module's struct.pack
and hashlib bytes (sst_encode_cases.py, whose coverage
tests/test_sst_encode_cases.py proves on the CPU), byte for byte: the smallest
shapes, the index step's edges, every length and alignment, every tile edge,
the committed golden table, a realistic batch that is flushed to a tree and
verified, shared sources, offsets across 2^32, the guards around both arenas,
every error, and the host form."""
import base64
import filecmp
import json
import os
import struct
import zlib

import numpy as np
import pytest

import sst_encode_cases as S
from lsm_storage_engine_amd import _lib, sstable
from lsm_storage_engine_amd.device import SstEncodeError
from oracle import oracle as O

pytestmark = pytest.mark.gpu
AA = 0xAA
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def T(ctx):
    t = ctx.get_stat("sst_encode_tile")
    assert t in S.TILES  # a power of two, 256 .. 65536: what the case tests cover
    return t


class DeviceBatch:
    """A batch's arenas and entries on the device, and output buffers filled
    with 0xAA: the data arena's base `shift` bytes past a multiple of T, GUARD
    bytes of the buffer (and more) in front of it and `slack` behind its
    capacity; the index arena, the spans and the digests each between GUARD
    bytes of 0xAA too."""

    def __init__(self, ctx, b, T, shift=0, data_cap=None, index_cap=None, slack=64, digests=True):
        self.ctx, self.b, self.n, self.ntab = ctx, b, len(b), b.ntab
        self.total, self.itotal = b.sizes_only()
        self.data_cap = self.total if data_cap is None else data_cap
        self.index_cap = self.itotal if index_cap is None else index_cap
        self.digests = digests
        self.bufs = []
        self.dk = self._up(b.keys)
        self.dv = self.dk if b.vals is b.keys else self._up(b.vals)
        self.de = self._up(b.ents)
        self.ddata = self._filled(S.GUARD + 2 * T + self.data_cap + slack)
        self.data_ptr = (self.ddata.ptr + S.GUARD + T - 1) // T * T + shift
        self.data_off = self.data_ptr - self.ddata.ptr
        self.dindex = self._filled(S.GUARD + self.index_cap + slack)
        self.dspans = self._filled(2 * S.GUARD + 32 * self.ntab)
        self.dsha = self._filled(3 * S.GUARD + 64 * self.ntab)
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

    def encode(self, data_cap=None, index_cap=None, first=None):
        b = self.b
        sha = self.dsha.ptr + S.GUARD
        return self.ctx.sstable_encode_batch_device(
            self.dk.ptr, b.keys.nbytes, self.dv.ptr, b.vals.nbytes, self.de.ptr, self.n,
            b.first if first is None else first, self.data_ptr, self.data_cap if data_cap is None else data_cap,
            self.dindex.ptr + S.GUARD, self.index_cap if index_cap is None else index_cap, self.dspans.ptr + S.GUARD,
            sha if self.digests else None, sha + 32 * self.ntab + S.GUARD if self.digests else None)

    def data(self, nbytes):
        return self.ddata.download(np.uint8, nbytes, self.data_off)

    def index(self, nbytes):
        return self.dindex.download(np.uint8, nbytes, S.GUARD)

    def spans(self):
        return self.dspans.download(_lib.SSTABLE_SPAN_DTYPE, self.ntab, S.GUARD)

    def shas(self):
        w = self.dsha.download()
        g, k = S.GUARD, 32 * self.ntab
        return w[g:g + k].reshape(-1, 32), w[2 * g + k:2 * g + 2 * k].reshape(-1, 32)

    def untouched_around(self, total, itotal, outputs=True):
        """Everything but data bytes [0, total), index bytes [0, itotal) and
        (outputs) the spans and digests is still 0xAA."""
        w, x = self.ddata.download(), self.dindex.download()
        ok = (w[:self.data_off] == AA).all() and (w[self.data_off + total:] == AA).all()
        ok = ok and (x[:S.GUARD] == AA).all() and (x[S.GUARD + itotal:] == AA).all()
        s, h = self.dspans.download(), self.dsha.download()
        g, k = S.GUARD, 32 * self.ntab
        if outputs:
            ok = ok and (s[:g] == AA).all() and (s[g + k:] == AA).all()
            ok = ok and (h[:g] == AA).all() and (h[g + k:2 * g + k] == AA).all() and (h[2 * g + 2 * k:] == AA).all()
            if not self.digests:
                ok = ok and (h == AA).all()
        else:
            ok = ok and (s == AA).all() and (h == AA).all()
        return bool(ok)

    def all_untouched(self):
        return self.untouched_around(0, 0, outputs=False)

    def free(self):
        for d in self.bufs:
            d.free()


def check(ctx, b, T, shift=0, extra_cap=0, digests=True):
    """Encode on the device and compare: both arenas, spans, digests, sizes, guards."""
    data, index, spans, dsha, isha = b.expected()
    d = DeviceBatch(ctx, b, T, shift, data_cap=len(data) + extra_cap, index_cap=len(index) + extra_cap,
                    digests=digests)
    try:
        assert d.encode() == (len(data), len(index))
        got = d.data(len(data))
        if not np.array_equal(got, data):
            off = b.rec_off()[0]
            bad = np.nonzero(got != data)[0]
            r = np.searchsorted(off, bad[:6], side="right") - 1
            raise AssertionError(f"{b}: shift {shift}: {len(bad)} data bytes differ, first at {bad[:6].tolist()} = "
                                 f"records {r.tolist()} + {(bad[:6] - off[r]).tolist()} (tile {T}: "
                                 f"{(bad[:6] + shift) % T})")
        assert np.array_equal(d.index(len(index)), index), f"{b}: the index arena differs"
        assert np.array_equal(d.spans(), spans)
        if digests:
            gd, gi = d.shas()
            assert np.array_equal(gd, dsha) and np.array_equal(gi, isha)
        assert d.untouched_around(len(data), len(index)), f"{b}: shift {shift}: bytes outside the outputs were written"
    finally:
        d.free()


# --- smallest shapes ---------------------------------------------------------
@pytest.mark.parametrize("i", range(4))
def test_one_table_of_one_entry(ctx, T, i):
    for shift in (0, 1, 3, 15):
        check(ctx, S.smallest()[i], T, shift)


def test_empty_tables(ctx, T):
    check(ctx, S.empty_tables(5), T)
    check(ctx, S.empty_tables(1), T, shift=3)
    check(ctx, S.empty_table_places(), T)
    check(ctx, S.empty_table_places(), T, shift=15)


def test_two_tables_in_one_chunk(ctx, T):
    for shift in (0, 1, 8, 15):
        check(ctx, S.two_in_a_chunk(), T, shift)


def test_nothing_at_all(ctx):
    none = np.zeros(0, np.uint8)
    data, index, spans, dsha, isha = ctx.sstable_encode_batch(none, none, np.zeros(0, _lib.WAL_CMD_DTYPE), [0])
    assert len(data) == len(index) == len(spans) == len(dsha) == len(isha) == 0
    assert ctx.sstable_encode_batch_device(0, 0, 0, 0, 0, 0, [0], 0, 0, 0, 0) == (0, 0)
    with pytest.raises(_lib.LsmckError) as e:  # a flag bit the call does not know
        ctx._sst_encode(0, 0, 0, 0, 0, 0, [0], 0, 0, 0, 0, None, None, None, _lib.DEVICE | 0x40)
    assert e.value.rc == _lib.EINVAL


# --- index step edges --------------------------------------------------------
def test_index_step_edges(ctx, T):
    b = S.index_steps()
    check(ctx, b, T)
    check(ctx, b, T, shift=3, digests=False)
    data, index, spans, _, _ = ctx.sstable_encode_batch(b.keys, b.vals, b.ents, b.first)
    counts = [struct.unpack_from("<Q", index, int(o))[0] for o in spans["index_off"]]
    assert counts == list(S.STEP_COUNTS)


# --- lengths and alignment ------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_lengths_and_alignments(ctx, T, shift):
    """Keys and values of 0..48 bytes at every source residue mod 16 and every
    destination residue, the data arena at base + 0, 1, 3, 15."""
    check(ctx, S.lengths_alignment(), T, shift, extra_cap=100)


# --- tile edges --------------------------------------------------------------------
def test_tile_edges_in_every_record_byte_and_at_a_table_start(ctx, T):
    check(ctx, S.tile_records(T), T)


@pytest.mark.parametrize("plus", [0, 1])
def test_arena_of_whole_tiles_and_one_byte_more(ctx, T, plus):
    check(ctx, S.tile_sized(T, 3, plus), T)
    check(ctx, S.tile_sized(T, 3, plus), T, shift=15)


# --- the golden table ---------------------------------------------------------------
def test_golden_table(ctx, T):
    """The entries parsed from the committed data file encode to that file, the
    committed index file and the committed checksum file's two strings."""
    want_data = open(os.path.join(GOLDEN, "sstable_test_data.db"), "rb").read()
    want_index = open(os.path.join(GOLDEN, "sstable_test_index.db"), "rb").read()
    js = json.load(open(os.path.join(GOLDEN, "sstable_test_checksum.db")))
    ko, kl, vo, vl, p = [], [], [], [], 0
    while p < len(want_data):
        k, v = struct.unpack_from("<II", want_data, p)
        ko.append(p + 8), kl.append(k), vo.append(p + 8 + k), vl.append(v)
        p += 8 + k + v
    assert len(ko) == 500
    arena = np.frombuffer(want_data, np.uint8)  # keys and values where the file holds them: one arena
    b = S.Batch("golden", arena, arena, S.entries(ko, kl, vo, vl), [0, 500])
    data, index, spans, dsha, isha = ctx.sstable_encode_batch(b.keys, b.keys, b.ents, b.first)
    assert data.tobytes() == want_data and index.tobytes() == want_index
    assert base64.b64encode(isha[0].tobytes()).decode() == js["index_checksum"]
    assert base64.b64encode(dsha[0].tobytes()).decode() == js["data_checksum"]
    check(ctx, b, T, shift=1)


# --- a realistic batch ----------------------------------------------------------------
def test_zipf_tables_flush_and_verify(ctx, T, tmp_path, monkeypatch):
    b = S.zipf_tables()
    assert len(b) == 200_000
    check(ctx, b, T)
    tables = [dict(b.table(t)) for t in range(b.ntab)]
    ts = [1_700_000_000_000 + t for t in range(b.ntab)]
    gpu, cpu = tmp_path / "gpu", tmp_path / "cpu"
    for where, c in ((cpu, None), (gpu, ctx)):
        os.makedirs(where)
        monkeypatch.chdir(where)  # (the metadata file names its base path: both trees are written as "tree")
        for lv in range(5):
            os.makedirs(os.path.join("tree", f"level-{lv}"))
        metas = sstable.flush_many("tree", 1, tables, c, ts)
        assert len(metas) == b.ntab
    rep = ctx.tree_verify("tree")  # (the verify follows the metadata's base path: the GPU's tree, from inside it)
    assert rep["tables"] == b.ntab and rep["bad_tables"] == 0
    g1, c1 = gpu / "tree" / "level-1", cpu / "tree" / "level-1"
    names = sorted(os.listdir(g1))
    assert len(names) == 5 * b.ntab and names == sorted(os.listdir(c1))
    match, mismatch, errors = filecmp.cmpfiles(g1, c1, names, shallow=False)
    assert not mismatch and not errors and len(match) == 5 * b.ntab


# --- shared and repeated sources ------------------------------------------------------
def test_keys_and_values_in_one_arena(ctx, T):
    b = S.shared_arena()
    assert b.vals is b.keys
    check(ctx, b, T)
    data, index, spans, dsha, isha = ctx.sstable_encode_batch(b.keys, b.keys, b.ents, b.first)  # the arena uploaded once
    e = b.expected()
    assert all(np.array_equal(x, y) for x, y in zip((data, index, spans, dsha, isha), e))


def test_many_entries_one_value(ctx, T):
    check(ctx, S.one_value(), T, shift=1)


# --- offsets across 2^32 ------------------------------------------------------------------
def test_offsets_across_4gib(ctx, T):
    """70 entries of one 64 MiB value, then 1000 small ones, in five tables:
    the data arena is ~4.4 GiB and is checked where it is -- spans, the index's
    pos values, every whole record's CRC-32 on the device against zlib's of the
    expected bytes -- and its small tail byte for byte.  No digests."""
    keys, ents, first = S.big_entries()
    n, nbig, ntab = len(ents), 70, len(first) - 1
    value = O.gen_stream(S.BIG_SEED, 0, S.BIG_VALUE)
    b = S.Batch("big", keys, value[:2048], ents, first)  # (sizes and the small entries' sources)
    off, total = b.rec_off()
    sizes = b.sizes()
    itotal = b.sizes_only()[1]
    assert total > 1 << 32
    bufs = [ctx.alloc(x) for x in (keys.nbytes, S.BIG_VALUE, ents.nbytes, total, itotal, 32 * ntab, 8 * n, 4 * n, 4 * n)]
    dk, dv, de, ddata, dindex, dspans, doff, dlen, dcrc = bufs
    try:
        dk.upload(keys)
        de.upload(ents)
        ctx.gen_stream(dv.ptr, S.BIG_SEED, 0, S.BIG_VALUE)
        ctx.sync()
        assert ctx.sstable_encode_batch_device(dk.ptr, keys.nbytes, dv.ptr, S.BIG_VALUE, de.ptr, n, first, ddata.ptr,
                                               total, dindex.ptr, itotal, dspans.ptr) == (total, itotal)
        # spans, and the index: count, then (8, key, pos) per 100th entry, pos inside the table's own file
        o = np.concatenate([off, [total]]).astype(np.uint64)
        spans = dspans.download(_lib.SSTABLE_SPAN_DTYPE, ntab)
        want_index = bytearray()
        for t in range(ntab):
            f0, f1 = int(first[t]), int(first[t + 1])
            assert (int(spans[t]["data_off"]), int(spans[t]["data_len"])) == (int(o[f0]), int(o[f1] - o[f0]))
            assert int(spans[t]["index_off"]) == len(want_index)
            want_index += struct.pack("<Q", (f1 - f0 + 99) // 100)
            for i in range(f0, f1, 100):
                want_index += struct.pack("<Q", 8) + b.key(i) + struct.pack("<Q", int(o[i] - o[f0]))
            assert int(spans[t]["index_len"]) == len(want_index) - int(spans[t]["index_off"])
        assert int(spans[2]["data_off"]) > 1 << 32 and len(want_index) == itotal
        assert dindex.download(np.uint8, itotal).tobytes() == bytes(want_index)
        # expected CRC of every whole record
        cv = zlib.crc32(value)
        want = np.empty(n, dtype=np.uint32)
        for i in range(n):
            k, vl, vo = b.key(i), int(ents["vlen"][i]), int(ents["val_off"][i])
            head = struct.pack("<II", len(k), vl) + k
            if i < nbig:
                want[i] = S.crc_concat(zlib.crc32(head), cv, vl)
            else:
                want[i] = zlib.crc32(head + value[vo:vo + vl].tobytes())
        doff.upload(off)
        dlen.upload(sizes.astype(np.uint32))
        ctx.crc32_device(ddata.ptr, doff.ptr, dlen.ptr, n, dcrc.ptr)
        ctx.sync()
        got = dcrc.download(np.uint32, n)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        # the small tail, byte for byte
        t0 = int(off[nbig])
        tail = b"".join(struct.pack("<II", 8, int(ents["vlen"][i])) + b.key(i) + b.val(i) for i in range(nbig, n))
        assert ddata.download(np.uint8, total - t0, t0).tobytes() == tail
    finally:
        for d in bufs:
            d.free()


def test_digest_of_a_table_above_4gib_is_refused(ctx, T):
    """A digest asked for a table whose data image is above 2^32-1 bytes:
    LSMCK_EINVAL with no entry to blame, nothing written; the sources are small
    (65 entries share one 64 MiB value) and no arena is needed for the refusal."""
    n = 65
    ents = S.entries(np.arange(n) * 8, [8] * n, [0] * n, [S.BIG_VALUE] * n)
    keys = S.counter_keys(n)
    bufs = [ctx.alloc(x) for x in (keys.nbytes, S.BIG_VALUE, ents.nbytes, 4096)]
    dk, dv, de, dout = bufs
    try:
        dk.upload(keys)
        de.upload(ents)
        ctx.memset(dout.ptr, AA, 4096)
        ctx.sync()
        with pytest.raises(SstEncodeError) as e:
            ctx.sstable_encode_batch_device(dk.ptr, keys.nbytes, dv.ptr, S.BIG_VALUE, de.ptr, n, [0, 1, n], dout.ptr,
                                            1 << 40, dout.ptr + 1024, 1024, dout.ptr + 2048, dout.ptr + 3072, None)
        assert e.value.rc == _lib.EINVAL and e.value.bad_index is None and "table 1" in str(e.value)
        assert (dout.download() == AA).all()
    finally:
        for d in bufs:
            d.free()


# --- errors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(10))
def test_invalid_entry_is_refused(ctx, T, case):
    name, args, idx, _ = S.invalid_cases()[case]
    b = S.Batch(name, *args)
    d = DeviceBatch(ctx, b, T, data_cap=4096, index_cap=4096)
    try:
        with pytest.raises(SstEncodeError) as e:
            d.encode()
        assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx, name
        assert d.all_untouched(), f"{name}: an output was written"
    finally:
        d.free()
    with pytest.raises(SstEncodeError) as e:  # the host form reports the same entry
        ctx.sstable_encode_batch(b.keys, b.vals, b.ents, b.first)
    assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx


def test_order_across_a_table_boundary_is_free(ctx, T):
    check(ctx, S.ok_across_boundary(), T)


def test_malformed_table_first_is_refused(ctx, T):
    b = S.ok_across_boundary()
    d = DeviceBatch(ctx, b, T, data_cap=4096, index_cap=4096)
    try:
        for name, first in S.bad_table_firsts(len(b)).items():
            with pytest.raises(SstEncodeError) as e:
                d.encode(first=np.array(first, dtype=np.uint64))
            assert e.value.rc == _lib.EINVAL and e.value.bad_index is None, name
        assert d.all_untouched()
    finally:
        d.free()


@pytest.mark.parametrize("short", ["data", "index"])
def test_short_buffer_is_enospc(ctx, T, short):
    b = S.empty_table_places()
    data, index, spans, dsha, isha = b.expected()
    total, itotal = len(data), len(index)
    d = DeviceBatch(ctx, b, T, data_cap=total - (short == "data"), index_cap=itotal - (short == "index"), slack=64)
    try:
        with pytest.raises(SstEncodeError) as e:
            d.encode()
        assert e.value.rc == _lib.ENOSPC and e.value.needed == (total, itotal) and e.value.bad_index is None
        assert d.all_untouched()
        # (the buffers hold `slack` more) and the context is fine afterwards
        assert d.encode(data_cap=total, index_cap=itotal) == (total, itotal)
        assert np.array_equal(d.data(total), data) and np.array_equal(d.index(itotal), index)
        gd, gi = d.shas()
        assert np.array_equal(gd, dsha) and np.array_equal(gi, isha)
    finally:
        d.free()


# --- host form ------------------------------------------------------------------------------------------
def test_host_form_equals_the_expected_bytes(ctx, T):
    b = S.lengths_alignment()
    e = b.expected()
    got = ctx.sstable_encode_batch(b.keys, b.vals, b.ents, b.first)  # pageable
    assert all(np.array_equal(x, y) for x, y in zip(got, e))
    got = ctx.sstable_encode_batch(b.keys, b.vals, b.ents, b.first, digests=False)
    assert got[3] is None and got[4] is None and all(np.array_equal(x, y) for x, y in zip(got[:3], e[:3]))
    pk, pv = ctx.alloc_pinned(b.keys.nbytes), ctx.alloc_pinned(b.vals.nbytes)
    try:
        pk.array[:], pv.array[:] = b.keys, b.vals
        got = ctx.sstable_encode_batch(pk.array, pv.array, b.ents, b.first, pinned=True)
        assert all(np.array_equal(x, y) for x, y in zip(got, e))
    finally:
        pk.free()
        pv.free()


def test_from_memtable_on_the_gpu_writes_the_golden_files(ctx, tmp_path):
    ents = dict((str(i).encode(), str(i * 100).encode()) for i in range(500))
    m = sstable.from_memtable(str(tmp_path), ents, ctx=ctx, timestamp_ms=1700000000000)
    for path, name in ((m.data_path(), "sstable_test_data.db"), (m.index_path(), "sstable_test_index.db"),
                       (m.checksum_path(), "sstable_test_checksum.db")):
        assert filecmp.cmp(path, os.path.join(GOLDEN, name), shallow=False), name
