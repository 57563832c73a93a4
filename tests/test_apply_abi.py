"""lsmck_db_apply_plan without a GPU: the call fails with LSMCK_ENODEV and
leaves its outputs defined, the arguments that are checked before any GPU work
are refused with or without one, the header and the binding agree on the two
calls, and the host helper lsmck_db_apply_plan_cpu gives the cases' expected
values (apply_cases.py) on every stream, errors and LSMCK_ENOSPC included.
No GPU compute call is made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import apply_cases as Ac
import write_cases as Wc
from lsm_storage_engine_amd import _lib

NONE = 2 ** 64 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Out:
    """cap entries, sources, Gets, miss queries and cap + 1 segments of 0xAA bytes; the five words set to 7."""

    def __init__(self, cap=16):
        def aa(nbytes, dtype):
            return np.full(nbytes, 0xAA, dtype=np.uint8).view(dtype)
        self.ents, self.src = aa(32 * cap, _lib.WAL_CMD_DTYPE), aa(4 * cap, np.uint32)
        self.segs, self.gets = aa(24 * (cap + 1), _lib.WRITE_SEG_DTYPE), aa(24 * cap, _lib.APPLY_GET_DTYPE)
        self.miss_q, self.miss_get = aa(16 * cap, _lib.GET_QUERY_DTYPE), aa(4 * cap, np.uint32)
        self.nent, self.nflush, self.nget, self.nmiss = (C.c_size_t(7) for _ in range(4))
        self.bad = C.c_uint64(7)

    def arrays(self):
        return self.ents, self.src, self.segs, self.gets, self.miss_q, self.miss_get

    def untouched(self, nent=0, nseg=0, nget=0, nmiss=0):
        cut = (nent, nent, nseg, nget, nmiss, nmiss)
        return all((a[k:].view(np.uint8) == 0xAA).all() for a, k in zip(self.arrays(), cut))

    def counts(self):
        return self.nent.value, self.nflush.value, self.nget.value, self.nmiss.value

    def words(self, **null):
        return [None if null.get(k) else C.byref(getattr(self, k)) for k in ("nent", "nflush", "nget", "nmiss", "bad")]


def call(s, o, flags, n=None, ctx=None, **null):
    g = s.g
    return _lib.load().lsmck_db_apply_plan(
        ctx, g.keys.ctypes.data, g.keys.nbytes, g.vals.ctypes.data, g.vals.nbytes, g.cmds.ctypes.data,
        len(g) if n is None else n, s.limit, s.tomb_off, o.ents.ctypes.data, len(o.ents), o.src.ctypes.data,
        o.segs.ctypes.data, len(o.segs), o.gets.ctypes.data, len(o.gets), None if null.get("miss_q") else o.miss_q.ctypes.data,
        None if null.get("miss_get") else o.miss_get.ctypes.data, *o.words(**null), flags)


def call_cpu(s, o, ent_cap=None, seg_cap=None, get_cap=None, tomb_off=None, vals=None, src=True, miss=True):
    g = s.g
    vals = g.vals if vals is None else vals
    return _lib.load().lsmck_db_apply_plan_cpu(
        g.keys.ctypes.data, g.keys.nbytes, vals.ctypes.data, vals.nbytes, g.cmds.ctypes.data, len(g), s.limit,
        s.tomb_off if tomb_off is None else tomb_off, o.ents.ctypes.data, len(o.ents) if ent_cap is None else ent_cap,
        o.src.ctypes.data if src else None, o.segs.ctypes.data, len(o.segs) if seg_cap is None else seg_cap,
        o.gets.ctypes.data, len(o.gets) if get_cap is None else get_cap, o.miss_q.ctypes.data if miss else None,
        o.miss_get.ctypes.data if miss else None, *o.words())


def test_without_a_gpu_the_call_fails_cleanly():
    lib = _lib.load()
    s, o = Ac.basic()[1], Out()
    rc = call(s, o, _lib.HOST)
    if lib.lsmck_device_count() == 0:
        assert rc == _lib.ENODEV and "no HIP device" in _lib.last_error()
    else:
        assert rc == _lib.EINVAL and "context" in _lib.last_error()
    assert o.counts() == (0, 0, 0, 0) and o.bad.value == NONE and o.untouched()


def test_arguments_checked_before_any_gpu_work():
    s = Ac.basic()[1]
    for flags in (0x40, _lib.DEVICE | 0x4, 0x80000000):
        o = Out()
        assert call(s, o, flags) == _lib.EINVAL and "flag" in _lib.last_error()
        assert o.counts() == (0, 0, 0, 0) and o.bad.value == NONE and o.untouched()
    for word in ("nent", "nflush", "nget", "nmiss"):
        o = Out()
        assert call(s, o, _lib.HOST, **{word: True}) == _lib.EINVAL and word in _lib.last_error() and o.untouched()
    for one in ("miss_q", "miss_get"):  # both or neither
        o = Out()
        assert call(s, o, _lib.HOST, **{one: True}) == _lib.EINVAL and "miss_q" in _lib.last_error() and o.untouched()
    for n in (1 << 32, 1 << 40):
        o = Out()
        assert call(s, o, _lib.HOST, n=n) == _lib.EINVAL and "2^32" in _lib.last_error() and o.untouched()
    o = Out()
    assert call(s, o, 0x40, bad=True) == _lib.EINVAL  # a null bad_index is allowed


def test_header_binding_and_export_agree():
    from lsm_storage_engine_amd import db, device
    header = open(os.path.join(ROOT, "include", "lsmck.h")).read()
    names = dict((sig[0], sig) for sig in _lib.SIGNATURES)
    for name, nargs in (("lsmck_db_apply_plan", 24), ("lsmck_db_apply_plan_cpu", 22)):
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == nargs == len(names[name][2])
        assert hasattr(_lib.load(), name)
    assert "#define LSMCK_CMD_GET 3u" in header and _lib.CMD_GET == 3
    assert "#define LSMCK_APPLY_MEMTABLE 0xFFFFFFFEu" in header and _lib.APPLY_MEMTABLE == 0xFFFFFFFE == Ac.MEMTABLE
    assert _lib.APPLY_GET_DTYPE.names == ("val_off", "vlen", "source", "cmd", "src_cmd")
    assert _lib.APPLY_GET_DTYPE.itemsize == 24 and "lsmck_apply_get;   /* 24 bytes */" in header
    assert "reads between the writes" not in header.split("lsmck_db_apply_plan's, below")[0].split("Not modelled")[-1]
    for attr in ("db_apply_plan", "db_apply_plan_device"):
        assert callable(getattr(device.Context, attr))
    e = device.ApplyPlanError(_lib.ENOSPC, "db_apply_plan", needed=(5, 2, 3, 1))
    assert (e.bad_index, e.needed, e.rc) == (None, (5, 2, 3, 1), _lib.ENOSPC) and isinstance(e, _lib.LsmckError)
    assert callable(db.apply_many) and {"apply_many", "Get"} <= set(db.__all__) and db.Get(b"k") == db.Get(b"k")


# --- the host helper -----------------------------------------------------------------------------
def check_cpu(s, **kw):
    p, answers = s.expected()
    o = Out(len(s) + 2)
    assert call_cpu(s, o, **kw) == 0, _lib.last_error()
    nmiss = sum(1 for a in answers if a.source == Ac.NONE)
    assert o.counts() == (len(p.entries), p.nflush, len(answers), nmiss) and o.bad.value == NONE
    e, k, g = len(p.entries), p.nflush + 1, len(answers)
    miss = kw.get("miss", True)
    Ac.check_outputs(s, o.ents[:e], o.src[:e], o.segs[:k], o.gets[:g], o.miss_q[:nmiss] if miss else None,
                     o.miss_get[:nmiss] if miss else None)
    assert o.untouched(e, k, g, nmiss if miss else 0)
    return o


@pytest.mark.parametrize("s", Ac.small() + Ac.scans() + Ac.wide() + [Ac.get_ignores_value_fields()], ids=lambda s: s.name)
def test_cpu_helper_equals_the_cases(s):
    check_cpu(s)


@pytest.mark.parametrize("s", Wc.smallest() + Wc.rule() + Wc.placement()[:6], ids=lambda s: s.name)
def test_cpu_helper_without_gets_is_the_write_plans_helper(s):
    """Byte-identical outputs on a stream without Gets."""
    lib, g, n = _lib.load(), s.g, len(s)
    o, w = Out(n + 2), Out(n + 2)
    args = (g.keys.ctypes.data, g.keys.nbytes, g.vals.ctypes.data, g.vals.nbytes, g.cmds.ctypes.data, n, s.limit, s.tomb_off)
    assert lib.lsmck_db_write_plan_cpu(*args, w.ents.ctypes.data, n + 2, w.src.ctypes.data, w.segs.ctypes.data, n + 3,
                                       C.byref(w.nent), C.byref(w.nflush), C.byref(w.bad)) == 0
    assert call_cpu(s, o) == 0
    assert o.counts() == (w.nent.value, w.nflush.value, 0, 0)
    for a, b in ((o.ents, w.ents), (o.src, w.src), (o.segs, w.segs)):
        assert a.tobytes() == b.tobytes()
    assert o.untouched(n + 2, n + 3, 0, 0)


def test_cpu_helper_optional_outputs():
    s = Ac.basic()[2]
    o = check_cpu(s, miss=False)
    assert (o.miss_q.view(np.uint8) == 0xAA).all() and (o.miss_get.view(np.uint8) == 0xAA).all()
    p = s.expected()[0]
    o = Out()
    assert call_cpu(s, o, src=False) == 0 and s.entries_of(o.ents[:len(p.entries)]) == p.entries
    assert (o.src.view(np.uint8) == 0xAA).all()


def test_cpu_helper_errors():
    for name, s, idx in Ac.invalid_cases():
        o = Out()
        assert call_cpu(s, o) == _lib.EINVAL, name
        assert o.bad.value == idx and o.counts() == (0, 0, 0, 0) and o.untouched()
    s = Ac.tombstones()[1]  # delete_flush_then_get
    p, answers = s.expected()
    one = s.g.vals.copy()
    one[s.tomb_off] = 1
    for kw in ({"vals": one}, {"tomb_off": len(s.g.vals)}, {"tomb_off": NONE}):  # not 0; past the arena
        o = Out()
        assert call_cpu(s, o, **kw) == _lib.EINVAL
        assert o.bad.value == NONE and "tomb" in _lib.last_error() and o.untouched()
    no_delete = Ac.basic()[2]  # no delete: the byte is not looked at
    assert call_cpu(no_delete, Out(), tomb_off=NONE) == 0
    nmiss = len(s.misses())
    need = (len(p.entries), p.nflush, len(answers), nmiss)
    for kw in ({"ent_cap": need[0] - 1}, {"seg_cap": need[1]}, {"get_cap": need[2] - 1}, {"get_cap": 0},
               {"ent_cap": 0, "seg_cap": 0, "get_cap": 0}):
        o = Out()
        assert call_cpu(s, o, **kw) == _lib.ENOSPC
        assert o.counts() == need and o.untouched()
    assert call_cpu(s, Out(), ent_cap=need[0], seg_cap=need[1] + 1, get_cap=need[2]) == 0


def test_cpu_helper_n0_and_only_gets():
    s = Ac.stream("n0", [], 10)
    o = check_cpu(s)
    assert o.segs[0].tolist() == (0, 0, 0)
    o = check_cpu(Ac.edges()[0])  # only Gets: one open segment, no entry
    assert o.segs[0].tolist() == (0, 0, 0) and o.counts() == (0, 0, 4, 4)
