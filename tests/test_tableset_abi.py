"""lsmck_tableset_open / _get_batch / _stat / _close without a GPU: open fails
with LSMCK_ENODEV, leaves *set NULL and its 0xAA-filled arenas untouched; the
arguments that are checked before any GPU work are refused with or without
one; close(NULL) is a no-op; and the binding's argument counts and names match
the header.  No GPU compute call is made here."""
import ctypes as C
import os
import re

import numpy as np

import get_cases as G
from lsm_storage_engine_amd import _lib

NONE = 2 ** 64 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_batch():
    tabs, keys = G.several_tables()
    return G.GetBatch([G.images(t) for t in tabs], keys)


def open_set(b, flags, ctx=None, ntab=None, data=True, index=True, spans=True, handle=True, bad=True):
    h, bt = C.c_void_p(0xAAAAAAAA), C.c_uint64(7)
    rc = _lib.load().lsmck_tableset_open(ctx, b.data.ctypes.data if data else None, b.data.nbytes,
                                         b.index.ctypes.data if index else None, b.index.nbytes,
                                         b.spans.ctypes.data if spans else None, len(b.spans) if ntab is None else ntab,
                                         C.byref(h) if handle else None, C.byref(bt) if bad else None, flags)
    return rc, h.value, bt.value


class Outputs:
    def __init__(self, n):
        self.res = np.full(16 * n, 0xAA, dtype=np.uint8)
        self.off = np.full(8 * (n + 1), 0xAA, dtype=np.uint8)
        self.out = np.full(4096, 0xAA, dtype=np.uint8)
        self.words = [C.c_uint64(7) for _ in range(3)]  # out_bytes, bad_run_entry, bad_query

    def untouched(self):
        return bool((self.res == 0xAA).all() and (self.off == 0xAA).all() and (self.out == 0xAA).all())


def get(b, o, flags, handle=None, ctx=None):
    w = [C.byref(x) for x in o.words]
    return _lib.load().lsmck_tableset_get_batch(ctx, handle, None, 0, b.qkeys.ctypes.data, b.qkeys.nbytes, b.q.ctypes.data,
                                                len(b.q), o.res.ctypes.data, o.out.ctypes.data, o.out.nbytes,
                                                o.off.ctypes.data, *w, flags)


def test_signatures_match_the_header():
    names = dict((s[0], s) for s in _lib.SIGNATURES)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsmck.h")).read(), flags=re.S)
    assert "typedef struct lsmck_tableset lsmck_tableset;" in txt
    want = {"lsmck_tableset_open": ("int", 10), "lsmck_tableset_get_batch": ("int", 16), "lsmck_tableset_stat": ("int", 3),
            "lsmck_tableset_close": ("void", 1)}
    for name, (ret, nargs) in want.items():
        proto = re.search(r"(\w+)\s+%s\((.*?)\);" % name, txt, flags=re.S)
        assert proto and proto.group(1) == ret and len(proto.group(2).split(",")) == nargs, name
        assert len(names[name][2]) == nargs and (names[name][1] is None) == (ret == "void"), name
    args = re.search(r"int lsmck_tableset_get_batch\((.*?)\);", txt, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "set", "runs", "nrun", "qkeys", "qkeys_bytes", "q", "n", "res", "out", "out_cap", "out_off", "out_bytes",
        "bad_run_entry", "bad_query", "flags"]
    # lsmck_db_get_batch's arguments but data .. ntab and bad_table, the set in their place
    db = re.search(r"int lsmck_db_get_batch\((.*?)\);", txt, flags=re.S).group(1)
    db = [a.split()[-1].lstrip("*") for a in db.split(",")]
    gone = ("data", "data_bytes", "index", "index_bytes", "spans", "ntab", "bad_table")
    mine = [a.split()[-1].lstrip("*") for a in args.split(",")]
    assert [a for a in db if a not in gone] == [a for a in mine if a != "set"]
    args = re.search(r"int lsmck_tableset_open\((.*?)\);", txt, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == [
        "ctx", "data", "data_bytes", "index", "index_bytes", "spans", "ntab", "set", "bad_table", "flags"]


def test_without_a_gpu_open_fails_cleanly():
    lib = _lib.load()
    want = _lib.ENODEV if lib.lsmck_device_count() == 0 else _lib.EINVAL
    word = "no HIP device" if want == _lib.ENODEV else "context"
    b = small_batch()
    data, index = b.data.copy(), b.index.copy()
    for flags in (_lib.HOST, _lib.DEVICE, _lib.HOST_PINNED):
        rc, h, bt = open_set(b, flags)
        assert rc == want and word in _lib.last_error() and h is None and bt == NONE
    rc, h, _ = open_set(b, _lib.HOST, bad=False)  # a null bad_table is allowed
    assert rc == want and h is None
    rc, h, _ = open_set(b, _lib.HOST, ntab=0, spans=False, index=False)  # the empty set needs a context too
    assert rc == want and h is None
    assert np.array_equal(data, b.data) and np.array_equal(index, b.index)
    # the get without a set: refused, its outputs still 0xAA
    for flags in (_lib.HOST, _lib.DEVICE):
        o = Outputs(len(b.q))
        assert get(b, o, flags) == _lib.EINVAL and "null set" in _lib.last_error()
        assert o.untouched() and [w.value for w in o.words] == [0, NONE, NONE]


def test_arguments_checked_before_any_gpu_work():
    b = small_batch()

    def refused(word, **kw):
        rc, h, bt = open_set(b, kw.pop("flags", _lib.HOST), **kw)
        assert rc == _lib.EINVAL and word in _lib.last_error(), (kw, _lib.last_error())
        assert h is None and bt == NONE, kw
    for flags in (0x40, _lib.DEVICE | 0x4, _lib.MERGE_DROP_TOMBSTONES, _lib.RECS_DEVICE, 0x80000000):
        refused("flag", flags=flags)
    for ntab in (1 << 32, (1 << 32) + 5, 1 << 40, 1 << 63):
        refused("2^32", ntab=ntab)
    refused("null index", index=False)
    refused("null", spans=False)
    refused("null", data=False)
    rc = _lib.load().lsmck_tableset_open(None, b.data.ctypes.data, b.data.nbytes, b.index.ctypes.data, b.index.nbytes,
                                         b.spans.ctypes.data, len(b.spans), None, None, _lib.HOST)
    assert rc == _lib.EINVAL and "null set" in _lib.last_error()


def test_close_null_and_stat_null():
    lib = _lib.load()
    lib.lsmck_tableset_close(None)
    lib.lsmck_tableset_close(None)
    v = C.c_long(5)
    assert lib.lsmck_tableset_stat(None, b"tables", C.byref(v)) == _lib.EINVAL and v.value == 5


def test_the_python_binding_names_the_calls():
    from lsm_storage_engine_amd import db, device
    assert callable(device.Context.tableset_open)
    for attr in ("get_batch", "get_batch_device", "stat", "close", "__enter__", "__exit__"):
        assert callable(getattr(device.TableSet, attr))
    for attr in ("get_many", "close"):
        assert callable(getattr(db.Reader, attr))
    assert "Reader" in db.__all__
