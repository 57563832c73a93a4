"""lsmck_db_get_batch without a GPU: the call fails with LSMCK_ENODEV and
leaves its 0xAA-filled outputs untouched, the arguments that are checked before
any GPU work are refused with or without one, and the binding's dtypes, argument
counts and names match the header.  No GPU compute call is made here."""
import ctypes as C
import os
import re

import numpy as np

import dbget_cases as D
import get_cases as G
from lsm_storage_engine_amd import _lib

NONE = 2 ** 64 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_batch():
    runs, tabs, keys = D.precedence()
    return D.DbGetBatch([D.Run(runs[0], 3, 5), D.Run(runs[1], 1, 2, one=True)], [G.images(t) for t in tabs], keys)


def descriptors(b):
    d = np.zeros(len(b.runs), dtype=_lib.GET_RUN_DTYPE)
    for r, run in enumerate(b.runs):
        d[r] = (run.keys.ctypes.data, run.keys.nbytes, run.vals.ctypes.data, run.vals.nbytes, run.ents.ctypes.data,
                len(run.ents))
    return d


class Outputs:
    def __init__(self, b):
        n = len(b.q)
        self.res = np.full(16 * n, 0xAA, dtype=np.uint8)
        self.off = np.full(8 * (n + 1), 0xAA, dtype=np.uint8)
        self.out = np.full(4096, 0xAA, dtype=np.uint8)
        self.words = [C.c_uint64(7) for _ in range(4)]  # out_bytes, bad_run_entry, bad_table, bad_query

    def untouched(self):
        return bool((self.res == 0xAA).all() and (self.off == 0xAA).all() and (self.out == 0xAA).all())

    def bad(self):
        return tuple(w.value for w in self.words[1:])


def db_get(b, o, flags, desc=None, nrun=None, ntab=None, n=None, ctx=None, runs=True, index=True, spans=True, q=True,
           results=True, out=True, out_off=True, out_bytes=True, bad=True):
    desc = descriptors(b) if desc is None else desc
    w = [C.byref(x) for x in o.words]
    return _lib.load().lsmck_db_get_batch(
        ctx, desc.ctypes.data if runs else None, len(desc) if nrun is None else nrun, b.data.ctypes.data, b.data.nbytes,
        b.index.ctypes.data if index else None, b.index.nbytes, b.spans.ctypes.data if spans else None,
        len(b.spans) if ntab is None else ntab, b.qkeys.ctypes.data, b.qkeys.nbytes, b.q.ctypes.data if q else None,
        len(b.q) if n is None else n, o.res.ctypes.data if results else None, o.out.ctypes.data if out else None,
        o.out.nbytes, o.off.ctypes.data if out_off else None, w[0] if out_bytes else None,
        *(w[1:] if bad else (None, None, None)), flags)


def test_dtypes_and_signature_match_the_header():
    assert _lib.GET_RUN_DTYPE == D.RUN_DTYPE and _lib.GET_RUN_DTYPE.itemsize == 48
    assert _lib.GET_RUN_DTYPE.names == ("keys", "keys_bytes", "vals", "vals_bytes", "ents", "nent")
    names = dict((s[0], s) for s in _lib.SIGNATURES)
    assert len(names["lsmck_db_get_batch"][2]) == 22 and len(names["lsmck_sstable_get_batch"][2]) == 15
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsmck.h")).read(), flags=re.S)
    proto = re.search(r"int lsmck_db_get_batch\((.*?)\);", txt, flags=re.S).group(1)
    assert len(proto.split(",")) == 22
    run = re.search(r"typedef struct \{([^}]*)\} lsmck_get_run;", txt).group(1)
    assert re.findall(r"(\w+);", run) == list(_lib.GET_RUN_DTYPE.names)


def test_without_a_gpu_the_call_fails_cleanly():
    lib = _lib.load()
    want = _lib.ENODEV if lib.lsmck_device_count() == 0 else _lib.EINVAL
    word = "no HIP device" if want == _lib.ENODEV else "context"
    b = small_batch()
    for flags in (_lib.HOST, _lib.DEVICE, _lib.HOST_PINNED):
        o = Outputs(b)
        assert db_get(b, o, flags) == want
        assert word in _lib.last_error() and o.bad() == (NONE, NONE, NONE) and o.words[0].value == 0 and o.untouched()
    o = Outputs(b)
    assert db_get(b, o, _lib.HOST, bad=False) == want and o.untouched()  # null bad words are allowed
    assert db_get(b, o, _lib.HOST, out=False, out_off=False, out_bytes=False) == want and o.untouched()  # no gather
    assert db_get(b, o, _lib.HOST, runs=False, nrun=0) == want and o.untouched()  # no runs


def refused(b, word, **kw):
    o = Outputs(b)
    assert db_get(b, o, kw.pop("flags", _lib.HOST), **kw) == _lib.EINVAL, kw
    assert word in _lib.last_error(), (_lib.last_error(), kw)
    assert o.bad() == (NONE, NONE, NONE) and o.untouched(), kw


def test_arguments_checked_before_any_gpu_work():
    b = small_batch()
    for flags in (0x40, _lib.DEVICE | 0x4, _lib.MERGE_DROP_TOMBSTONES, _lib.RECS_DEVICE, 0x80000000):
        refused(b, "flag", flags=flags)
    for kw in (dict(n=1 << 32), dict(ntab=1 << 32), dict(nrun=1 << 32), dict(n=(1 << 32) + 5), dict(ntab=1 << 40),
               dict(n=1 << 63)):
        refused(b, "2^32", **kw)
    d = descriptors(b)
    d["nent"][1] = 1 << 32
    refused(b, "2^32", desc=d)
    d["nent"] = [(1 << 31) + 1, 1 << 31]  # (together)
    refused(b, "2^32", desc=d)
    refused(b, "null runs", runs=False)
    refused(b, "null index", index=False)
    for kw in (dict(spans=False), dict(q=False), dict(results=False)):
        refused(b, "null", **kw)
    for field in ("ents", "keys", "vals"):
        d = descriptors(b)
        d[field][1] = 0
        refused(b, "null", desc=d)
    refused(b, "out_bytes", out_bytes=False)
    refused(b, "null out", out=False)


def test_the_python_binding_names_the_calls():
    from lsm_storage_engine_amd import db, device
    for attr in ("db_get_batch", "db_get_batch_device"):
        assert callable(getattr(device.Context, attr))
    e = device.DbGetError(_lib.EINVAL, "db_get_batch", bad_run_entry=3)
    assert (e.bad_run_entry, e.bad_table, e.bad_query, e.needed, e.rc) == (3, None, None, None, _lib.EINVAL)
    e = device.DbGetError(_lib.ENOSPC, "db_get_batch", needed=99)
    assert (e.bad_run_entry, e.needed) == (None, 99) and isinstance(e, _lib.LsmckError)
    assert callable(db.get_many) and db.TOMBSTONE_HIT is not None
    # without a context db.get_many is the literal loop
    mem, old = {b"a": b"1", b"gone": b"\x00"}, {b"a": b"old", b"b": b"2", b"gone": b"back"}
    assert db.get_many([mem, old], [], [b"a", b"b", b"gone", b"c"]) == [b"1", b"2", None, None]
    assert db.get_many([mem, old], [], [b"gone"], internal=True) == [db.TOMBSTONE_HIT]
    arena, vals, ents = db.run_arrays(old)
    assert vals is arena and arena.tobytes() == b"aoldb2goneback" and ents["key_off"].tolist() == [0, 4, 6]
