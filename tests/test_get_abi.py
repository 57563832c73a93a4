"""lsmck_sstable_get_batch without a GPU -- the call fails with LSMCK_ENODEV and
leaves its outputs defined, and the arguments that are checked before any GPU
work are refused with or without one -- and lsmck_sstable_get (scalar, no GPU:
the code the kernels share, lsmck_sstget.h) against the cases module on every
case of tests/get_cases.py.  No GPU compute call is made here."""
import ctypes as C

import numpy as np

import get_cases as G
from lsm_storage_engine_amd import _lib

NONE = 2 ** 64 - 1


def small_batch():
    tabs, keys = G.several_tables()
    return G.GetBatch([G.images(t) for t in tabs], keys)


def get_batch(b, res, bad_t, bad_q, flags, ntab=None, n=None, ctx=None, index=True, spans=True, q=True, results=True):
    return _lib.load().lsmck_sstable_get_batch(
        ctx, b.data.ctypes.data, b.data.nbytes, b.index.ctypes.data if index else None, b.index.nbytes,
        b.spans.ctypes.data if spans else None, len(b.spans) if ntab is None else ntab, b.qkeys.ctypes.data,
        b.qkeys.nbytes, b.q.ctypes.data if q else None, len(b.q) if n is None else n,
        res.ctypes.data if results else None, bad_t, bad_q, flags)


def outputs(b):
    return np.full(16 * len(b.q), 0xAA, dtype=np.uint8), C.c_uint64(7), C.c_uint64(7)


def test_dtypes_and_constants_match_the_header():
    assert _lib.GET_QUERY_DTYPE == G.QUERY_DTYPE and _lib.GET_RESULT_DTYPE == G.RESULT_DTYPE
    assert (_lib.GET_NONE, _lib.GET_TOMBSTONE) == (G.NONE_TABLE, G.TOMBSTONE_BIT)
    names = dict((s[0], s) for s in _lib.SIGNATURES)
    assert len(names["lsmck_sstable_get_batch"][2]) == 15 and len(names["lsmck_sstable_get"][2]) == 8


def test_without_a_gpu_the_batch_call_fails_cleanly():
    lib = _lib.load()
    want = _lib.ENODEV if lib.lsmck_device_count() == 0 else _lib.EINVAL
    word = "no HIP device" if want == _lib.ENODEV else "context"
    b = small_batch()
    res, bt, bq = outputs(b)
    assert get_batch(b, res, C.byref(bt), C.byref(bq), _lib.HOST) == want
    assert word in _lib.last_error() and (bt.value, bq.value) == (NONE, NONE) and (res == 0xAA).all()
    assert get_batch(b, res, C.byref(bt), C.byref(bq), _lib.DEVICE) == want and (res == 0xAA).all()
    assert get_batch(b, res, None, None, _lib.HOST) == want  # null bad words are allowed


def test_arguments_checked_before_any_gpu_work():
    b = small_batch()
    for flags in (0x40, _lib.DEVICE | 0x4, _lib.MERGE_DROP_TOMBSTONES, _lib.RECS_DEVICE, 0x80000000):
        res, bt, bq = outputs(b)
        assert get_batch(b, res, C.byref(bt), C.byref(bq), flags) == _lib.EINVAL
        assert "flag" in _lib.last_error() and (bt.value, bq.value) == (NONE, NONE) and (res == 0xAA).all()
    for kw in (dict(n=1 << 32), dict(ntab=1 << 32), dict(n=(1 << 32) + 5), dict(ntab=1 << 40), dict(n=1 << 63)):
        res, bt, bq = outputs(b)
        assert get_batch(b, res, C.byref(bt), C.byref(bq), _lib.HOST, **kw) == _lib.EINVAL, kw
        assert "2^32" in _lib.last_error() and (bt.value, bq.value) == (NONE, NONE) and (res == 0xAA).all()
    res, bt, bq = outputs(b)
    assert get_batch(b, res, C.byref(bt), C.byref(bq), _lib.HOST, index=False) == _lib.EINVAL
    assert "null index" in _lib.last_error() and (bt.value, bq.value) == (NONE, NONE) and (res == 0xAA).all()
    for kw in (dict(spans=False), dict(q=False), dict(results=False)):
        res, bt, bq = outputs(b)
        assert get_batch(b, res, C.byref(bt), C.byref(bq), _lib.HOST, **kw) == _lib.EINVAL, kw
        assert "null" in _lib.last_error() and (bt.value, bq.value) == (NONE, NONE) and (res == 0xAA).all()


def scalar_get(data, index, key):
    """lsmck_sstable_get over exact-size copies: None, (offset, value), or "refused"."""
    lib = _lib.load()
    d, x, k = (np.frombuffer(bytes(s), dtype=np.uint8).copy() for s in (data, index, key))
    off, vlen = C.c_uint64(NONE), C.c_uint32(77)
    rc = lib.lsmck_sstable_get(d.ctypes.data if len(d) else None, len(d), x.ctypes.data if len(x) else None, len(x),
                               k.ctypes.data if len(k) else None, len(k), C.byref(off), C.byref(vlen))
    if rc == 0 or rc == _lib.EINVAL:
        assert (off.value, vlen.value) == (0, 0)
        return None if rc == 0 else "refused"
    assert rc == 1
    return off.value, bytes(data[off.value:off.value + vlen.value])


def test_scalar_get_on_the_sized_and_tie_tables():
    for name, ents, step in [(n, e, 100) for n, e in G.sized_tables()] + G.tie_tables():
        data, index = G.images(ents, step)
        m = G.btreemap(index)
        for k in G.queries_for(ents):
            assert scalar_get(data, index, k) == G.table_get(data, index, k, m), (name, k)


def test_scalar_get_on_the_quirks_and_cuts():
    absent = [b"", b"q", b"q00100x", b"q0010", b"q00150xx\x00", b"q00099xxx\x00", b"zzz", b"q00249x\x00"]
    for name, (data, index) in G.quirk_tables().items():
        m = G.btreemap(index)
        for k in [e[0] for e in G.QUIRK_ENTRIES] + absent:
            assert scalar_get(data, index, k) == G.table_get(data, index, k, m), (name, k)
    for cut, (data, index), ents in G.cut_tables():
        for k in [e[0] for e in ents] + [b"c9", b"", b"c4yyy"]:
            assert scalar_get(data, index, k) == G.table_get(data, index, k), (cut, k)


def test_scalar_get_refuses_what_the_cases_refuse():
    data = G.data_image(G.QUIRK_ENTRIES)
    for name, x in G.refused_indexes():
        assert scalar_get(data, x, G.QUIRK_ENTRIES[7][0]) == "refused", name
        assert "index" in _lib.last_error()
    ents, bad = G.refused_fixed_indexes()
    for name, x in bad:
        assert scalar_get(G.data_image(ents), x, ents[7][0]) == "refused", name
    lib = _lib.load()
    off, vlen = C.c_uint64(9), C.c_uint32(9)
    x = np.frombuffer(G.index_image([]), dtype=np.uint8)
    assert lib.lsmck_sstable_get(None, 1 << 32, x.ctypes.data, len(x), None, 0, C.byref(off), C.byref(vlen)) == _lib.EINVAL
    assert "2^32" in _lib.last_error() and (off.value, vlen.value) == (0, 0)
    assert lib.lsmck_sstable_get(None, 0, x.ctypes.data, len(x), None, 0, None, C.byref(vlen)) == _lib.EINVAL
    assert lib.lsmck_sstable_get(None, 0, x.ctypes.data, len(x), None, 0, C.byref(off), C.byref(vlen)) == 0


def test_scalar_get_on_several_tables_and_the_seeded_batch():
    tabs, keys = G.several_tables()
    for t in tabs:
        data, index = G.images(t)
        for k in keys:
            assert scalar_get(data, index, k) == G.table_get(data, index, k), k
    # the seeded batch: every query against every table, the expected value from the dict form that
    # tests/test_get_cases.py proves equal to the restatement on such tables
    tabs, keys = G.seeded_batch()
    lib = _lib.load()
    karr = [np.frombuffer(k, dtype=np.uint8) for k in sorted(set(keys))]
    off, vlen = C.c_uint64(), C.c_uint32()
    for ents in tabs:
        data, index = G.images(ents)
        d, x = np.frombuffer(data, dtype=np.uint8), np.frombuffer(index, dtype=np.uint8)
        want, pos = {}, 0
        for k, v in ents:
            want[k] = (pos + 8 + len(k), len(v))
            pos += 8 + len(k) + len(v)
        for ka in karr:
            rc = lib.lsmck_sstable_get(d.ctypes.data, len(d), x.ctypes.data, len(x), ka.ctypes.data, len(ka),
                                       C.byref(off), C.byref(vlen))
            w = want.get(ka.tobytes())
            assert (rc, off.value, vlen.value) == ((0, 0, 0) if w is None else (1,) + w)


def test_the_python_binding_names_the_calls():
    from lsm_storage_engine_amd import device, sstable
    for attr in ("sstable_get_batch", "sstable_get_batch_device"):
        assert callable(getattr(device.Context, attr))
    e = device.SstGetError(_lib.EINVAL, "sstable_get_batch", bad_table=3)
    assert (e.bad_table, e.bad_query, e.rc) == (3, None, _lib.EINVAL) and isinstance(e, _lib.LsmckError)
    e = device.SstGetError(_lib.EINVAL, "sstable_get_batch", bad_query=5)
    assert (e.bad_table, e.bad_query) == (None, 5)
    assert callable(sstable.table_get) and callable(sstable.get_many) and sstable.TOMBSTONE_HIT is not None
    data, index = G.images(G.QUIRK_ENTRIES)
    assert sstable.table_get(data, index, b"q00150xx") == b"val-150" and sstable.table_get(data, index, b"q") is None
