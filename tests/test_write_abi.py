"""lsmck_db_write_plan without a GPU: the call fails with LSMCK_ENODEV and
leaves its outputs defined, the arguments that are checked before any GPU work
are refused with or without one, and the binding names the call.  Then the
host helper lsmck_db_write_plan_cpu -- the scalar fallback -- against the
cases' restatement (write_cases.plan) on every stream but the 2^18-command
one, the window and wide-block streams among them, its errors included.  No GPU compute call is made here."""
import ctypes as C

import numpy as np
import pytest

import write_cases as Wc
from lsm_storage_engine_amd import _lib

NONE = 2 ** 64 - 1


def outputs(cap=16):
    """cap entries, sources and cap + 1 segments of 0xAA bytes; nent, nflush and bad_index set to 7."""
    return (np.full(32 * cap, 0xAA, dtype=np.uint8).view(_lib.WAL_CMD_DTYPE), np.full(cap, 0xAAAAAAAA, dtype=np.uint32),
            np.full(24 * (cap + 1), 0xAA, dtype=np.uint8).view(_lib.WRITE_SEG_DTYPE), C.c_size_t(7), C.c_size_t(7),
            C.c_uint64(7))


def untouched(ents, src, segs):
    return (ents.view(np.uint8) == 0xAA).all() and (src == 0xAAAAAAAA).all() and (segs.view(np.uint8) == 0xAA).all()


def call(s, ents, src, segs, nent, nflush, bad, flags, n=None, ctx=None):
    g = s.g
    return _lib.load().lsmck_db_write_plan(ctx, g.keys.ctypes.data, g.keys.nbytes, g.vals.ctypes.data, g.vals.nbytes,
                                           g.cmds.ctypes.data, len(g) if n is None else n, s.limit, s.tomb_off,
                                           ents.ctypes.data, len(ents), src.ctypes.data, segs.ctypes.data, len(segs),
                                           nent, nflush, bad, flags)


def call_cpu(s, ents, src, segs, nent, nflush, bad, ent_cap=None, seg_cap=None, tomb_off=None, vals=None):
    g = s.g
    vals = g.vals if vals is None else vals
    return _lib.load().lsmck_db_write_plan_cpu(
        g.keys.ctypes.data, g.keys.nbytes, vals.ctypes.data, vals.nbytes, g.cmds.ctypes.data, len(g), s.limit,
        s.tomb_off if tomb_off is None else tomb_off, ents.ctypes.data, len(ents) if ent_cap is None else ent_cap,
        None if src is None else src.ctypes.data, segs.ctypes.data, len(segs) if seg_cap is None else seg_cap,
        nent, nflush, bad)


def test_without_a_gpu_the_plan_fails_cleanly():
    lib = _lib.load()
    s = Wc.rule()[0]
    ents, src, segs, nent, nflush, bad = outputs()
    rc = call(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad), _lib.HOST)
    if lib.lsmck_device_count() == 0:
        assert not lib.lsmck_ctx_create(0)  # (there is no context to call with)
        assert rc == _lib.ENODEV and "no HIP device" in _lib.last_error()
    else:
        assert rc == _lib.EINVAL and "context" in _lib.last_error()
    assert (nent.value, nflush.value, bad.value) == (0, 0, NONE) and untouched(ents, src, segs)


def test_arguments_checked_before_any_gpu_work():
    s = Wc.rule()[0]
    for flags in (0x40, _lib.DEVICE | 0x4, _lib.RECS_DEVICE, 0x80000000):  # an unknown flag
        ents, src, segs, nent, nflush, bad = outputs()
        assert call(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad), flags) == _lib.EINVAL
        assert "flag" in _lib.last_error() and untouched(ents, src, segs)
        assert (nent.value, nflush.value, bad.value) == (0, 0, NONE)
    ents, src, segs, nent, nflush, bad = outputs()
    assert call(s, ents, src, segs, None, C.byref(nflush), C.byref(bad), _lib.HOST) == _lib.EINVAL  # a null nent
    assert "nent" in _lib.last_error() and nflush.value == 0 and untouched(ents, src, segs)
    assert call(s, ents, src, segs, C.byref(nent), None, C.byref(bad), _lib.HOST) == _lib.EINVAL
    assert "nflush" in _lib.last_error() and nent.value == 0
    for n in (1 << 32, (1 << 32) + 5, 1 << 40):  # n >= 2^32 (no command is read)
        ents, src, segs, nent, nflush, bad = outputs()
        assert call(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad), _lib.HOST, n=n) == _lib.EINVAL
        assert "2^32" in _lib.last_error() and untouched(ents, src, segs)
    # a null bad_index is allowed
    ents, src, segs, nent, nflush, bad = outputs()
    assert call(s, ents, src, segs, C.byref(nent), C.byref(nflush), None, 0x40) == _lib.EINVAL


def test_the_python_binding_names_the_calls():
    from lsm_storage_engine_amd import db, device
    names = dict((s[0], s) for s in _lib.SIGNATURES)
    assert len(names["lsmck_db_write_plan"][2]) == 18 and len(names["lsmck_db_write_plan_cpu"][2]) == 16
    assert _lib.WRITE_SEG_DTYPE.names == ("first_cmd", "first_ent", "mem_bytes") and _lib.WRITE_SEG_DTYPE.itemsize == 24
    for attr in ("db_write_plan", "db_write_plan_device"):
        assert callable(getattr(device.Context, attr))
    e = device.WritePlanError(_lib.ENOSPC, "db_write_plan", needed=(5, 2))
    assert (e.bad_index, e.needed, e.rc) == (None, (5, 2), _lib.ENOSPC) and isinstance(e, _lib.LsmckError)
    assert callable(db.write_many) and "write_many" in db.__all__


# --- the host helper -----------------------------------------------------------------------------
def check_cpu(s):
    p = s.expected()
    n = len(s)
    ents, src, segs, nent, nflush, bad = outputs(n + 2)
    assert call_cpu(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad)) == 0
    assert (nent.value, nflush.value, bad.value) == (len(p.entries), p.nflush, NONE)
    e, k = nent.value, nflush.value + 1
    assert [tuple(x) for x in segs[:k].tolist()] == p.segs and src[:e].tolist() == p.src
    assert s.entries_of(ents[:e]) == p.entries
    assert (ents["type"][:e] == 1).all() and (ents["reserved"][:e] == 0).all()
    dels = s.g.cmds["type"][src[:e]] == 2
    assert (ents["val_off"][:e][dels] == s.tomb_off).all() and (ents["vlen"][:e][dels] == 1).all()
    assert untouched(ents[e:], src[e:], segs[k:])


@pytest.mark.parametrize("s", Wc.smallest() + Wc.rule() + Wc.placement() + [Wc.sized(n, Wc.CAP) for n in (63, 1025)] +
                         Wc.windows() + Wc.wide(), ids=lambda s: s.name)
def test_cpu_helper_equals_the_restatement(s):
    check_cpu(s)


def test_cpu_helper_errors():
    for name, s, idx in Wc.invalid_cases():
        ents, src, segs, nent, nflush, bad = outputs()
        assert call_cpu(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad)) == _lib.EINVAL, name
        assert bad.value == idx and (nent.value, nflush.value) == (0, 0) and untouched(ents, src, segs)
    s = Wc.rule()[6]  # delete_last_writer
    p = s.expected()
    one = s.g.vals.copy()
    one[s.tomb_off] = 1
    for kw in ({"vals": one}, {"tomb_off": len(s.g.vals)}, {"tomb_off": NONE}):  # not 0; past the arena
        ents, src, segs, nent, nflush, bad = outputs()
        assert call_cpu(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad), **kw) == _lib.EINVAL
        assert bad.value == NONE and "tomb" in _lib.last_error() and untouched(ents, src, segs)
    inserts = Wc.rule()[2]  # no delete: the byte is not looked at
    ents, src, segs, nent, nflush, bad = outputs()
    assert call_cpu(inserts, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad), tomb_off=NONE) == 0
    for kw in ({"ent_cap": len(p.entries) - 1}, {"seg_cap": p.nflush}, {"ent_cap": 0, "seg_cap": 0}):
        ents, src, segs, nent, nflush, bad = outputs()
        assert call_cpu(s, ents, src, segs, C.byref(nent), C.byref(nflush), C.byref(bad), **kw) == _lib.ENOSPC
        assert (nent.value, nflush.value) == (len(p.entries), p.nflush) and untouched(ents, src, segs)
    ents, src, segs, nent, nflush, bad = outputs()  # src is optional
    assert call_cpu(s, ents, None, segs, C.byref(nent), C.byref(nflush), C.byref(bad)) == 0
    assert s.entries_of(ents[:nent.value]) == p.entries and (src == 0xAAAAAAAA).all()
