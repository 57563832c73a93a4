"""lsmck_memtable_build and lsmck_wal_recs_to_cmds without a GPU: the calls
fail with LSMCK_ENODEV and leave their outputs defined, and the arguments that
are checked before any GPU work are refused with or without one.  No GPU
compute call is made here."""
import ctypes as C

import numpy as np

import memtable_cases as M
from lsm_storage_engine_amd import _lib


def call(g, ents, src, nent, nbytes, bad, flags, n=None, ctx=None):
    return _lib.load().lsmck_memtable_build(ctx, g.keys.ctypes.data, g.keys.nbytes, g.vals.ctypes.data, g.vals.nbytes,
                                            g.cmds.ctypes.data, len(g) if n is None else n, ents.ctypes.data, len(ents),
                                            src.ctypes.data, nent, nbytes, bad, flags)


def outputs():
    """16 entries and sources of 0xAA bytes; nent, mem_bytes and bad_index set to 7."""
    return (np.full(32 * 16, 0xAA, dtype=np.uint8).view(_lib.WAL_CMD_DTYPE),
            np.full(16, 0xAAAAAAAA, dtype=np.uint32), C.c_size_t(7), C.c_uint64(7), C.c_uint64(7))


def untouched(ents, src):
    return (ents.view(np.uint8) == 0xAA).all() and (src == 0xAAAAAAAA).all()


def test_without_a_gpu_the_build_fails_cleanly():
    lib = _lib.load()
    g = M.smallest()[4]
    ents, src, nent, nbytes, bad = outputs()
    if lib.lsmck_device_count() == 0:
        assert not lib.lsmck_ctx_create(0)  # (there is no context to call with)
        rc = call(g, ents, src, C.byref(nent), C.byref(nbytes), C.byref(bad), _lib.HOST)
        assert rc == _lib.ENODEV and "no HIP device" in _lib.last_error()
        assert (nent.value, nbytes.value, bad.value) == (0, 0, 2 ** 64 - 1) and untouched(ents, src)
        assert lib.lsmck_wal_recs_to_cmds(None, ents.ctypes.data, 1, 100, ents.ctypes.data, None) == _lib.ENODEV
        assert untouched(ents, src)
    else:
        rc = call(g, ents, src, C.byref(nent), C.byref(nbytes), C.byref(bad), _lib.HOST)
        assert rc == _lib.EINVAL and "context" in _lib.last_error() and untouched(ents, src)


def test_arguments_checked_before_any_gpu_work():
    g = M.smallest()[4]
    for flags in (0x40, _lib.DEVICE | 0x4, _lib.RECS_DEVICE, 0x80000000):  # an unknown flag
        ents, src, nent, nbytes, bad = outputs()
        assert call(g, ents, src, C.byref(nent), C.byref(nbytes), C.byref(bad), flags) == _lib.EINVAL
        assert "flag" in _lib.last_error() and untouched(ents, src)
        assert (nent.value, nbytes.value, bad.value) == (0, 0, 2 ** 64 - 1)
    ents, src, nent, nbytes, bad = outputs()
    assert call(g, ents, src, None, C.byref(nbytes), C.byref(bad), _lib.HOST) == _lib.EINVAL  # a null nent
    assert "nent" in _lib.last_error() and nbytes.value == 0 and untouched(ents, src)
    assert call(g, ents, src, C.byref(nent), None, C.byref(bad), _lib.HOST) == _lib.EINVAL
    for n in (1 << 32, (1 << 32) + 5, 1 << 40):  # n >= 2^32 (no command is read)
        ents, src, nent, nbytes, bad = outputs()
        assert call(g, ents, src, C.byref(nent), C.byref(nbytes), C.byref(bad), _lib.HOST, n=n) == _lib.EINVAL
        assert "2^32" in _lib.last_error() and untouched(ents, src)
    # a null bad_index is allowed
    ents, src, nent, nbytes, bad = outputs()
    assert call(g, ents, src, C.byref(nent), C.byref(nbytes), None, 0x40) == _lib.EINVAL


def test_the_python_binding_names_the_calls():
    from lsm_storage_engine_amd import device, sstable, wal
    names = dict((s[0], s) for s in _lib.SIGNATURES)
    assert len(names["lsmck_memtable_build"][2]) == 14 and len(names["lsmck_wal_recs_to_cmds"][2]) == 6
    for attr in ("memtable_build", "memtable_build_device", "wal_recs_to_cmds_device"):
        assert callable(getattr(device.Context, attr))
    e = device.MemBuildError(_lib.EINVAL, "memtable_build", bad_index=3)
    assert (e.bad_index, e.needed, e.rc) == (3, None, _lib.EINVAL) and isinstance(e, _lib.LsmckError)
    assert callable(wal.MemTable.from_image) and callable(sstable.flush_log_image)
