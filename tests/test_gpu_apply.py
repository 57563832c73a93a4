"""lsmck_db_apply_plan on the GPU against the cases module's expected values
(apply_cases.py: "the last write in front", which tests/test_apply_cases.py
proves equal to the literal loop on the CPU): the write plan's outputs and the
LONG count, the Gets, the misses' queries and their indices; the six outputs
between 0xAA guards that must stay intact, as must everything past the counts.
The streams run with cut_block 64 and the stream's cut_walk_cap (4 or 64);
the wide streams at cut_block 8192.  In the same test the write plan's own
call runs over the stream without its Gets and must give the same entries and
segments after renumbering, byte for byte on a stream without Gets.  Then the
capacities and errors, the host form, and db.apply_many against the literal
loop over a base of two levels opened as a Reader."""
import filecmp
import os

import numpy as np
import pytest

import apply_cases as Ac
import memtable_cases as M
import write_cases as Wc
from lsm_storage_engine_amd import _lib, db, sstable, wal
from lsm_storage_engine_amd.device import ApplyPlanError

pytestmark = pytest.mark.gpu
AA = 0xAA
G = M.GUARD
SIZES = (32, 4, 24, 24, 16, 4)  # ents, src, segs, gets, miss_q, miss_get
DTYPES = (_lib.WAL_CMD_DTYPE, np.uint32, _lib.WRITE_SEG_DTYPE, _lib.APPLY_GET_DTYPE, _lib.GET_QUERY_DTYPE, np.uint32)


@pytest.fixture(autouse=True)
def default_options(ctx):
    yield
    ctx.set_option("cut_block", Wc.DEFAULT_BLOCK)
    ctx.set_option("cut_walk_cap", Wc.DEFAULT_CAP)


class DevicePlan:
    """A stream's arenas (each allocated at exactly its size) and commands on
    the device, and the six outputs, each between GUARD bytes of 0xAA and
    filled with 0xAA: ents and src of `cap` items, segs of `seg_cap`, gets,
    miss_q and miss_get of `get_cap`."""

    def __init__(self, ctx, s, cap=None, seg_cap=None, get_cap=None):
        self.ctx, self.s, self.n = ctx, s, len(s)
        self.cap = self.n + 3 if cap is None else cap
        self.seg_cap = self.n + 2 if seg_cap is None else seg_cap
        self.get_cap = self.n + 1 if get_cap is None else get_cap
        self.bufs = []
        g = s.g
        self.dk, self.dv, self.dc = self._up(g.keys), self._up(g.vals), self._up(g.cmds)
        caps = (self.cap, self.cap, self.seg_cap, self.get_cap, self.get_cap, self.get_cap)
        self.out = [self._filled(2 * G + size * c) for size, c in zip(SIZES, caps)]
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

    def options(self):
        self.ctx.set_option("cut_block", self.s.block)
        self.ctx.set_option("cut_walk_cap", self.s.cap)

    def run(self, cap=None, seg_cap=None, get_cap=None, src=True, miss=True, tomb_off=None, vals_bytes=None):
        s, g = self.s, self.s.g
        self.options()
        p = [d.ptr + G for d in self.out]
        return self.ctx.db_apply_plan_device(
            self.dk.ptr, g.keys.nbytes, self.dv.ptr, g.vals.nbytes if vals_bytes is None else vals_bytes, self.dc.ptr,
            self.n, s.limit, s.tomb_off if tomb_off is None else tomb_off, p[0], self.cap if cap is None else cap,
            p[1] if src else None, p[2], self.seg_cap if seg_cap is None else seg_cap, p[3],
            self.get_cap if get_cap is None else get_cap, p[4] if miss else None, p[5] if miss else None)

    def outputs(self, nent=0, nseg=0, nget=0, nmiss=0):
        """(the six arrays cut to the counts, whether every other byte of the six buffers is still 0xAA)."""
        counts, arrays, ok = (nent, nent, nseg, nget, nmiss, nmiss), [], True
        for d, size, dt, k in zip(self.out, SIZES, DTYPES, counts):
            b = d.download()
            ok = ok and bool((b[:G] == AA).all() and (b[G + size * k:] == AA).all())
            arrays.append(b[G:G + size * k].view(dt))
        return arrays, ok

    def free(self):
        for d in self.bufs:
            d.free()


def write_plan_of_the_erased(ctx, s):
    """lsmck_db_write_plan over the stream without its Gets: (ents, src, segs) in the full stream's numbers."""
    e, keep = s.erased()
    n = len(e)
    bufs = [ctx.alloc(max(a.nbytes, 1)) for a in (e.g.keys, e.g.vals, e.g.cmds)]
    outs = [ctx.alloc(max(size * c, 1)) for size, c in ((32, n), (4, n), (24, n + 1))]
    try:
        for b, a in zip(bufs, (e.g.keys, e.g.vals, e.g.cmds)):
            if a.nbytes:
                b.upload(a)
        ctx.set_option("cut_block", s.block)
        ctx.set_option("cut_walk_cap", s.cap)
        nent, nflush = ctx.db_write_plan_device(bufs[0].ptr, e.g.keys.nbytes, bufs[1].ptr, e.g.vals.nbytes, bufs[2].ptr, n,
                                                s.limit, s.tomb_off, outs[0].ptr, n, outs[1].ptr, outs[2].ptr, n + 1)
        ents = outs[0].download(_lib.WAL_CMD_DTYPE, nent) if nent else np.zeros(0, _lib.WAL_CMD_DTYPE)
        src = outs[1].download(np.uint32, nent) if nent else np.zeros(0, np.uint32)
        segs = outs[2].download(_lib.WRITE_SEG_DTYPE, nflush + 1)
        return ents, src, segs, keep
    finally:
        for b in bufs + outs:
            b.free()


def check_stream(ctx, s, erased=True, **caps):
    p, answers = s.expected()
    nmiss = len(s.misses())
    want = (len(p.entries), p.nflush, len(answers), nmiss)
    d = DevicePlan(ctx, s, **caps)
    try:
        got = d.run()
        steps, nlong = ctx.get_stat("cut_steps"), ctx.get_stat("cut_long")
        print(s.name, "nent, nflush, nget, nmiss:", got, "expected:", want, "cut_steps, cut_long:", steps, nlong,
              p.long_count(s.cap), "mem_rounds:", ctx.get_stat("mem_rounds"))
        assert got == want
        assert (ctx.get_stat("apply_gets"), ctx.get_stat("apply_misses")) == want[2:]
        (ents, src, segs, gets, miss_q, miss_get), guards = d.outputs(want[0], want[1] + 1, want[2], want[3])
        assert guards
        Ac.check_outputs(s, ents, src, segs, gets, miss_q, miss_get)
        assert nlong == p.long_count(s.cap) and steps <= len(s) * s.cap
        if erased:  # agreement with the write plan's own call on the remaining commands
            wents, wsrc, wsegs, keep = write_plan_of_the_erased(ctx, s)
            assert ents.tobytes() == wents.tobytes() and src.tolist() == keep[wsrc].tolist()
            assert segs["first_ent"].tolist() == wsegs["first_ent"].tolist()
            assert segs["mem_bytes"].tolist() == wsegs["mem_bytes"].tolist()
            first = [0] + [int(keep[c - 1]) + 1 for c in wsegs["first_cmd"].tolist()[1:]]
            assert segs["first_cmd"].tolist() == first
            if not s.is_get.any():
                assert src.tobytes() == wsrc.tobytes() and segs.tobytes() == wsegs.tobytes()
        return ents.copy(), src.copy(), segs.copy(), gets.copy(), miss_q.copy(), miss_get.copy()
    finally:
        d.free()


SMALL = Ac.small() + [Ac.get_ignores_value_fields(), Ac.stream("n0", [], 10)]


@pytest.mark.parametrize("s", [s.at(cap=cap, name=f"{s.name}@{cap}") for s in SMALL for cap in (Wc.CAP_SMALL, Wc.CAP)],
                         ids=lambda s: s.name)
def test_stream(ctx, s):
    check_stream(ctx, s)


@pytest.mark.parametrize("s", Ac.scans(), ids=lambda s: s.name)
def test_scans_across_workgroups(ctx, s):
    check_stream(ctx, s)


@pytest.mark.parametrize("s", Ac.wide(), ids=lambda s: s.name)
def test_wide_blocks_and_windows_with_gets(ctx, s):
    assert s.block == Wc.DEFAULT_BLOCK
    check_stream(ctx, s)


@pytest.mark.parametrize("s", Wc.smallest() + Wc.rule() + Wc.placement()[:8] + [Wc.sized(1025, Wc.CAP)], ids=lambda s: s.name)
def test_without_gets_the_outputs_are_the_write_plans(ctx, s):
    t = Ac.Stream.__new__(Ac.Stream)
    t.__dict__.update(s.__dict__)
    t._plan = None
    assert not t.is_get.any()
    check_stream(ctx, t)


def test_twice_gives_the_same_bytes(ctx):
    s = Ac.sized(4097, Wc.CAP)
    a = check_stream(ctx, s, erased=False)
    b = check_stream(ctx, s, erased=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_exact_caps_without_src_and_without_miss_arrays(ctx):
    s = Ac.sized(1023, Wc.CAP)
    p, answers = s.expected()
    want = (len(p.entries), p.nflush, len(answers), len(s.misses()))
    d = DevicePlan(ctx, s, cap=want[0], seg_cap=want[1] + 1, get_cap=want[2])
    try:
        assert d.run(src=False, miss=False) == want  # nmiss is reported without the arrays
        (ents, _, segs, gets, _, _), _ = d.outputs(want[0], want[1] + 1, want[2], 0)
        Ac.check_outputs(s, ents, np.array(p.src, dtype=np.uint32), segs, gets)
        full = [x.download() for x in d.out]
        assert (full[1] == AA).all() and (full[4] == AA).all() and (full[5] == AA).all()
        for k in (0, 2, 3):
            size, cnt = SIZES[k], (want[0], 0, want[1] + 1, want[2])[k]
            assert (full[k][:G] == AA).all() and (full[k][G + size * cnt:] == AA).all()
    finally:
        d.free()


# --- capacities and errors -------------------------------------------------------------------
def test_enospc_for_each_capacity(ctx):
    s = Ac.sized(1025, Wc.CAP)
    p, answers = s.expected()
    need = (len(p.entries), p.nflush, len(answers), len(s.misses()))
    d = DevicePlan(ctx, s)
    try:
        for kw in ({"cap": need[0] - 1}, {"cap": 0}, {"seg_cap": need[1]}, {"seg_cap": 0}, {"get_cap": need[2] - 1},
                   {"get_cap": 0}, {"cap": 0, "seg_cap": 0, "get_cap": 0}):
            with pytest.raises(ApplyPlanError) as e:
                d.run(**kw)
            assert e.value.rc == _lib.ENOSPC and e.value.needed == need and e.value.bad_index is None
            assert d.outputs()[1]
        assert d.run(cap=need[0], seg_cap=need[1] + 1, get_cap=need[2]) == need
    finally:
        d.free()


@pytest.mark.parametrize("case", Ac.invalid_cases(), ids=lambda c: c[0])
def test_invalid_command(ctx, case):
    name, s, idx = case
    d = DevicePlan(ctx, s)
    try:
        with pytest.raises(ApplyPlanError) as e:
            d.run()
        assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx and e.value.needed is None
        assert d.outputs()[1]
    finally:
        d.free()


def test_tombstone_byte(ctx):
    s = Ac.tombstones()[1]
    assert s.name == "delete_flush_then_get"
    one = Ac.tombstones()[1]
    one.g.vals[one.tomb_off] = 1
    for t, tomb_off, vals_bytes in ((one, None, None), (s, len(s.g.vals), None), (s, 2 ** 64 - 1, None),
                                    (s, None, s.tomb_off)):  # not 0; past the arena, by offset and by size
        d = DevicePlan(ctx, t)
        try:
            with pytest.raises(ApplyPlanError) as e:
                d.run(tomb_off=tomb_off, vals_bytes=vals_bytes)
            assert e.value.rc == _lib.EINVAL and e.value.bad_index is None and "tomb" in str(e.value)
            assert d.outputs()[1]
        finally:
            d.free()
    no_delete = Ac.basic()[2]  # no delete in the stream: the byte is not looked at
    p, answers = no_delete.expected()
    d = DevicePlan(ctx, no_delete)
    try:
        assert d.run(tomb_off=2 ** 64 - 1)[:3] == (len(p.entries), p.nflush, len(answers))
    finally:
        d.free()


# --- the host form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [Ac.sized(4097, Wc.CAP), Ac.stream("n0", [], 10), Ac.edges()[0], Ac.edges()[3],
                               Ac.tombstones()[2], Ac.tombstones()[1]], ids=lambda s: s.name)
def test_host_form_equals_the_device_form(ctx, s):
    dev = check_stream(ctx, s, erased=False)
    for pinned in (False, True):
        ctx.set_option("cut_block", s.block)
        ctx.set_option("cut_walk_cap", s.cap)
        got = ctx.db_apply_plan(s.g.keys, s.g.vals, s.g.cmds, s.limit, s.tomb_off, pinned=pinned)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, dev))
        Ac.check_outputs(s, *got)
    name, bad, idx = Ac.invalid_cases()[1]
    with pytest.raises(ApplyPlanError) as e:
        ctx.db_apply_plan(bad.g.keys, bad.g.vals, bad.g.cmds, bad.limit, bad.tomb_off)
    assert e.value.bad_index == idx
    if (s.g.cmds["type"] == 2).any():
        one = s.g.vals.copy()
        one[s.tomb_off] = 9
        with pytest.raises(ApplyPlanError) as e:
            ctx.db_apply_plan(s.g.keys, one, s.g.cmds, s.limit, s.tomb_off)
        assert e.value.rc == _lib.EINVAL and e.value.bad_index is None


# --- the pipeline ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bloom_bits", [0, 12])
def test_apply_many_equals_the_literal_loop(ctx, tmp_path, bloom_bits):
    # the base: two levels, keys the stream reads and never writes among them, one tombstone that answers
    old = {b"key-%d" % i: b"old-%d" % i for i in range(0, 960, 3)}
    new = {b"key-%d" % i: b"new-%d" % i for i in range(0, 960, 7)}
    new[b"key-21"] = db.DELETED
    levels = []
    for lvl, d in ((0, new), (1, old)):
        mt = wal.MemTable()
        for k in sorted(d):
            mt.insert(k, d[k])
        levels.append(sstable.flush_many(str(tmp_path / "base"), lvl, [mt], None, [1600000000000 + lvl]))
    commands = Ac.pipeline_commands()
    n_flush = Ac.literal(commands, 4096)[0].nflush
    stamps = [1700000000000 + 7 * i for i in range(n_flush)]
    a, b = tmp_path / "gpu", tmp_path / "host"
    with db.Reader(levels, ctx, bloom_bits=bloom_bits) as reader:
        for internal in (False, True):
            got = db.apply_many(str(a / str(internal)), commands, 4096, ctx=ctx, reader=reader, timestamps_ms=stamps,
                                internal=internal)
            want = db.apply_many(str(b / str(internal)), commands, 4096, ctx=None, reader=reader, timestamps_ms=stamps,
                                 internal=internal)
            assert got[0] == want[0] and len(want[0]) > 1500
            assert len(got[1]) == len(want[1]) == n_flush and n_flush > 5
            for m, w in zip(got[1], want[1]):
                for x, y in ((m.data_path(), w.data_path()), (m.index_path(), w.index_path()),
                             (m.checksum_path(), w.checksum_path())):
                    assert os.path.basename(x) == os.path.basename(y) and filecmp.cmp(x, y, shallow=False), x
            assert got[2].data == want[2].data and got[2].bytes == want[2].bytes and len(want[2].data) > 0
            assert got[3] == want[3] and len(want[3]) > 0
        # the base answered some Gets, a tombstone of it among them, and some Gets nobody answers
        hits = [r for r in want[0] if isinstance(r, bytes) and r[:4] in (b"old-", b"new-")]
        assert len(hits) > 20 and any(r is sstable.TOMBSTONE_HIT for r in want[0]) and any(r is None for r in want[0])
        # ... and the writes alone are write_many's
        writes = [c for c in commands if not isinstance(c, db.Get)]
        wm = db.write_many(str(tmp_path / "writes"), writes, 4096, ctx=ctx, timestamps_ms=stamps)
        assert wm[1].data == got[2].data and wm[2] == got[3] and len(wm[0]) == n_flush
