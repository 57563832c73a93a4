"""lsmck_db_write_plan on the GPU against the cases module's expected values
(write_cases.py: wal.MemTable.insert command by command, whose meaning
tests/test_write_cases.py proves on the CPU): the segments, the entries as (key
bytes, value bytes) through the arenas, src, nent, nflush and the LONG count;
the three outputs between 0xAA guards that must stay intact, as must
everything past the counts.  The streams run with cut_block 64 and the
stream's cut_walk_cap (4, 64 or the default 4096), so that a few hundred
commands reach the blocks' and the cap's edges; one case of 377 commands and
the pipeline run at the default cut_block 8192.  Blocks of up to 8192
starts, block widths that are no power of two and LONG memtables of more than
one of the chain's windows are test_gpu_write_plan_wide.py's.  Then the host
form, and db.write_many against the literal loop's files."""
import filecmp
import os

import numpy as np
import pytest

import memtable_cases as M
import write_cases as Wc
from lsm_storage_engine_amd import _lib, db, wal
from lsm_storage_engine_amd.device import WritePlanError

pytestmark = pytest.mark.gpu
AA = 0xAA
G = M.GUARD


@pytest.fixture(autouse=True)
def default_options(ctx):
    yield
    ctx.set_option("cut_block", Wc.DEFAULT_BLOCK)
    ctx.set_option("cut_walk_cap", Wc.DEFAULT_CAP)


class DevicePlan:
    """A stream's arenas (each allocated at exactly its size) and commands on
    the device, and the three outputs -- ents and src of `cap` entries, segs of
    `seg_cap` items -- each between GUARD bytes of 0xAA and filled with 0xAA."""

    def __init__(self, ctx, s, cap=None, seg_cap=None):
        self.ctx, self.s, self.n = ctx, s, len(s)
        self.cap = self.n + 3 if cap is None else cap
        self.seg_cap = self.n + 2 if seg_cap is None else seg_cap
        self.bufs = []
        g = s.g
        self.dk, self.dv, self.dc = self._up(g.keys), self._up(g.vals), self._up(g.cmds)
        self.dents = self._filled(2 * G + 32 * self.cap)
        self.dsrc = self._filled(2 * G + 4 * self.cap)
        self.dsegs = self._filled(2 * G + 24 * self.seg_cap)
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

    def run(self, cap=None, seg_cap=None, src=True, tomb_off=None, vals_bytes=None):
        s, g = self.s, self.s.g
        self.ctx.set_option("cut_block", s.block)
        self.ctx.set_option("cut_walk_cap", s.cap)
        return self.ctx.db_write_plan_device(
            self.dk.ptr, g.keys.nbytes, self.dv.ptr, g.vals.nbytes if vals_bytes is None else vals_bytes, self.dc.ptr,
            self.n, s.limit, s.tomb_off if tomb_off is None else tomb_off, self.dents.ptr + G,
            self.cap if cap is None else cap, self.dsrc.ptr + G if src else None, self.dsegs.ptr + G,
            self.seg_cap if seg_cap is None else seg_cap)

    def outputs(self, nent, nseg):
        """(ents[:nent], src[:nent], segs[:nseg]) and whether every other byte of the three buffers is still 0xAA."""
        e, s, q = self.dents.download(), self.dsrc.download(), self.dsegs.download()
        ok = (e[:G] == AA).all() and (e[G + 32 * nent:] == AA).all() and (s[:G] == AA).all() and \
            (s[G + 4 * nent:] == AA).all() and (q[:G] == AA).all() and (q[G + 24 * nseg:] == AA).all()
        return (e[G:G + 32 * nent].view(_lib.WAL_CMD_DTYPE), s[G:G + 4 * nent].view(np.uint32),
                q[G:G + 24 * nseg].view(_lib.WRITE_SEG_DTYPE), bool(ok))

    def free(self):
        for d in self.bufs:
            d.free()


def check_stream(ctx, s, cap=None, seg_cap=None):
    p = s.expected()
    d = DevicePlan(ctx, s, cap, seg_cap)
    try:
        got = d.run()
        steps, nlong = ctx.get_stat("cut_steps"), ctx.get_stat("cut_long")
        print(s.name, "nent, nflush:", got, "cut_steps, cut_long:", steps, nlong, "expected:", len(p.entries), p.nflush,
              p.long_count(s.cap))
        assert got == (len(p.entries), p.nflush)
        ents, src, segs, guards = d.outputs(got[0], got[1] + 1)
        assert guards
        assert [tuple(x) for x in segs.tolist()] == p.segs
        assert src.tolist() == p.src
        assert (ents["type"] == 1).all() and (ents["reserved"] == 0).all()
        assert s.entries_of(ents) == p.entries
        dels = s.g.cmds["type"][src] == 2
        assert (ents["val_off"][dels] == s.tomb_off).all() and (ents["vlen"][dels] == 1).all()
        assert nlong == p.long_count(s.cap) and steps <= len(s) * s.cap
        return ents.copy(), src.copy(), segs.copy()
    finally:
        d.free()


@pytest.mark.parametrize("s", Wc.smallest() + Wc.rule() + Wc.placement(), ids=lambda s: s.name)
def test_stream(ctx, s):
    check_stream(ctx, s)


def test_no_cut_is_the_single_memtable_with_tombstones(ctx):
    s = Wc.smallest()[10]
    assert s.name == "no_cut"
    ents, src, segs = check_stream(ctx, s)
    mt = wal.MemTable()
    for r in s.g.records():
        mt.insert(r.key, r.val if isinstance(r, wal.Insert) else db.DELETED)
    assert s.entries_of(ents) == sorted(mt.data.items()) and segs.tolist() == [(0, 0, mt.bytes)]


@pytest.mark.parametrize("cap", [Wc.CAP_SMALL, Wc.CAP])
@pytest.mark.parametrize("n", M.SIZES)
def test_sizes(ctx, n, cap):
    check_stream(ctx, Wc.sized(n, cap), cap=n, seg_cap=n + 1)


@pytest.mark.parametrize("limit", Wc.BIG_LIMITS)
def test_big(ctx, limit):
    """2^18 commands over 2^12 keys; UINT64_MAX is the all-LONG case: one memtable, found on the chain."""
    check_stream(ctx, Wc.big(limit))


def test_big_twice(ctx):
    a = check_stream(ctx, Wc.big(4096))
    b = check_stream(ctx, Wc.big(4096))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_default_options_and_exact_caps_without_src(ctx):
    s = Wc.placement()[3].at(cap=Wc.DEFAULT_CAP)
    s.block = Wc.DEFAULT_BLOCK
    p = s.expected()
    d = DevicePlan(ctx, s, cap=len(p.entries), seg_cap=p.nflush + 1)
    try:
        assert d.run(src=False) == (len(p.entries), p.nflush)
        ents, _, segs, _ = d.outputs(len(p.entries), p.nflush + 1)
        assert s.entries_of(ents) == p.entries and [tuple(x) for x in segs.tolist()] == p.segs
        assert (d.dsrc.download() == AA).all()
        e, q = d.dents.download(), d.dsegs.download()
        assert (e[:G] == AA).all() and (e[G + 32 * len(p.entries):] == AA).all()
        assert (q[:G] == AA).all() and (q[G + 24 * (p.nflush + 1):] == AA).all()
    finally:
        d.free()


# --- errors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Wc.invalid_cases(), ids=lambda c: c[0])
def test_invalid_command(ctx, case):
    name, s, idx = case
    d = DevicePlan(ctx, s)
    try:
        with pytest.raises(WritePlanError) as e:
            d.run()
        assert e.value.rc == _lib.EINVAL and e.value.bad_index == idx and e.value.needed is None
        assert d.outputs(0, 0)[3]
    finally:
        d.free()


def test_tombstone_byte(ctx):
    s = Wc.rule()[6]
    assert s.name == "delete_last_writer"
    one = Wc.rule()[6]
    one.g.vals[one.tomb_off] = 1
    for t, tomb_off, vals_bytes in ((one, None, None), (s, len(s.g.vals), None), (s, 2 ** 64 - 1, None),
                                    (s, None, s.tomb_off)):  # not 0; past the arena, by offset and by size
        d = DevicePlan(ctx, t)
        try:
            with pytest.raises(WritePlanError) as e:
                d.run(tomb_off=tomb_off, vals_bytes=vals_bytes)
            assert e.value.rc == _lib.EINVAL and e.value.bad_index is None and "tomb" in str(e.value)
            assert d.outputs(0, 0)[3]
        finally:
            d.free()
    inserts = Wc.rule()[2]  # no delete in the batch: the byte is not looked at
    p = inserts.expected()
    d = DevicePlan(ctx, inserts)
    try:
        assert d.run(tomb_off=2 ** 64 - 1) == (len(p.entries), p.nflush)
        ents, src, segs, guards = d.outputs(len(p.entries), p.nflush + 1)
        assert guards and inserts.entries_of(ents) == p.entries and src.tolist() == p.src
    finally:
        d.free()


def test_enospc(ctx):
    s = Wc.sized(1023, Wc.CAP)
    p = s.expected()
    d = DevicePlan(ctx, s)
    try:
        for kw in ({"cap": len(p.entries) - 1}, {"cap": 0}, {"seg_cap": p.nflush}, {"seg_cap": 0},
                   {"cap": 0, "seg_cap": 0}):
            with pytest.raises(WritePlanError) as e:
                d.run(**kw)
            assert e.value.rc == _lib.ENOSPC and e.value.needed == (len(p.entries), p.nflush)
            assert e.value.bad_index is None and d.outputs(0, 0)[3]
        assert d.run(cap=len(p.entries), seg_cap=p.nflush + 1) == (len(p.entries), p.nflush)
    finally:
        d.free()


# --- the host form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [Wc.sized(4097, Wc.CAP), Wc.smallest()[0], Wc.smallest()[8], Wc.rule()[6],
                               Wc.placement()[3]], ids=lambda s: s.name)
def test_host_form_equals_the_device_form(ctx, s):
    p = s.expected()
    dev = check_stream(ctx, s)
    for pinned in (False, True):
        ctx.set_option("cut_block", s.block)
        ctx.set_option("cut_walk_cap", s.cap)
        ents, src, segs = ctx.db_write_plan(s.g.keys, s.g.vals, s.g.cmds, s.limit, s.tomb_off, pinned=pinned)
        assert ents.tobytes() == dev[0].tobytes() and src.tolist() == p.src and segs.tobytes() == dev[2].tobytes()
        assert s.entries_of(ents) == p.entries
    name, bad, idx = Wc.invalid_cases()[4]
    with pytest.raises(WritePlanError) as e:
        ctx.db_write_plan(bad.g.keys, bad.g.vals, bad.g.cmds, bad.limit, bad.tomb_off)
    assert e.value.bad_index == idx
    one = s.g.vals.copy()
    one[s.tomb_off] = 9
    if (s.g.cmds["type"] == 2).any():
        with pytest.raises(WritePlanError) as e:
            ctx.db_write_plan(s.g.keys, one, s.g.cmds, s.limit, s.tomb_off)
        assert e.value.rc == _lib.EINVAL and e.value.bad_index is None


# --- the pipeline ----------------------------------------------------------------------------------------
def test_write_many_writes_the_literal_loops_files(ctx, tmp_path):
    commands = Wc.pipeline_commands()
    a, b = tmp_path / "gpu", tmp_path / "host"
    n_flush = len(Wc.plan(commands, 4096).segs) - 1
    stamps = [1700000000000 + 7 * i for i in range(n_flush)]
    got = db.write_many(str(a), commands, 4096, ctx=ctx, timestamps_ms=stamps)
    want = db.write_many(str(b), commands, 4096, ctx=None, timestamps_ms=stamps)
    assert len(got[0]) == len(want[0]) == n_flush and n_flush > 50
    for m, w in zip(got[0], want[0]):
        for x, y in ((m.data_path(), w.data_path()), (m.index_path(), w.index_path()),
                     (m.checksum_path(), w.checksum_path())):
            assert os.path.basename(x) == os.path.basename(y) and filecmp.cmp(x, y, shallow=False), x
    assert got[1].data == want[1].data and got[1].bytes == want[1].bytes and len(want[1].data) > 0
    assert got[2] == want[2] and len(want[2]) > 0
    replay = wal.MemTable()  # the log left is the memtable left
    for r in wal.CommandLog.new_in_memory(got[2]):
        replay.insert(r.key, r.val if isinstance(r, wal.Insert) else db.DELETED)
    assert replay.data == got[1].data and replay.bytes == got[1].bytes
    rep = ctx.tree_verify(str(a))
    assert rep["tables"] == n_flush and rep["bad_tables"] == 0
    model = {}
    for c in commands:
        model[c.key] = c.val if isinstance(c, wal.Insert) else None
    keys = sorted(model) + [b"key-absent"]
    want_vals = [model.get(k) for k in keys]
    assert db.get_many([got[1]], [got[0]], keys, ctx=ctx) == want_vals
    assert db.get_many([want[1]], [want[0]], keys[::37], ctx=None) == want_vals[::37]
