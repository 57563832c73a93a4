"""GPU context and batch entry points (include/lsmck.h sections 2-4).

``Context`` owns one liblsmck context (one MI355X).  Host-array methods take
numpy arrays and return numpy arrays (the library stages them through pinned
memory); ``*_device`` methods take raw device pointers (ints) and run
asynchronously on ``stream`` (a hipStream_t as int, or None for the context's
stream) -- that is the device-resident hot path the bench times.

There is no CPU fallback: constructing a Context without a usable gfx950 GPU
raises.
"""
import ctypes as C
import sys

import numpy as np

from . import _lib
from .shard import shard_by_bytes, shard_fixed


def _p(a):
    return None if a is None else a.ctypes.data


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = nbytes
        self.ptr = _lib.load().lsmck_dev_alloc(ctx.handle, nbytes)
        if not self.ptr:
            raise MemoryError(f"hipMalloc({nbytes}): {_lib.last_error()}")

    def free(self):
        if self.ptr:
            _lib.load().lsmck_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        assert offset + a.nbytes <= self.nbytes
        _lib.check(_lib.load().lsmck_memcpy_h2d(self.ctx.handle, self.ptr + offset, a.ctypes.data, a.nbytes, None),
                   "h2d")

    def download(self, dtype=np.uint8, count=None, offset=0):
        dt = np.dtype(dtype)
        count = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(count, dtype=dt)
        _lib.check(_lib.load().lsmck_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr + offset, out.nbytes, None),
                   "d2h")
        return out

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedBuffer:
    """Page-locked host memory (hipHostMalloc through liblsmck); ``array`` is a
    uint8 numpy view.  Batch calls given these arrays with pinned=True DMA
    straight from / to them (LSMCK_HOST_PINNED)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = nbytes
        self.ptr = _lib.load().lsmck_host_alloc_pinned(ctx.handle, max(1, nbytes))
        if not self.ptr:
            raise MemoryError(f"hipHostMalloc({nbytes}): {_lib.last_error()}")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(self.ptr))[:nbytes]

    def free(self):
        if self.ptr:
            self.array = None
            _lib.load().lsmck_host_free_pinned(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _PinnedRecords:
    """numpy's view of a PinnedBuffer as lsmck_wal_rec[n] (or another record
    dtype): the arrays made from it keep it (and the page-locked memory) alive."""

    def __init__(self, pb, n, dtype):
        self.pb = pb
        self.__array_interface__ = {"data": (pb.ptr, False), "shape": (n,), "typestr": dtype.str,
                                    "descr": dtype.descr, "version": 3}


class WalEncodeError(_lib.LsmckError):
    """lsmck_wal_encode_batch refused the batch: ``bad_index`` is the first
    invalid command (LSMCK_EINVAL), or ``needed`` the image's size when the
    buffer given is smaller (LSMCK_ENOSPC); the other one is None."""

    def __init__(self, rc, what, bad_index=None, needed=None):
        self.bad_index = bad_index
        self.needed = needed
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed})")


class SstEncodeError(_lib.LsmckError):
    """lsmck_sstable_encode_batch refused the batch: ``bad_index`` is the first
    offending entry (LSMCK_EINVAL; None when the error is table_first's or a
    table too long to hash), or ``needed`` = (data bytes, index bytes) when a
    buffer given is smaller (LSMCK_ENOSPC); the other one is None."""

    def __init__(self, rc, what, bad_index=None, needed=None):
        self.bad_index = bad_index
        self.needed = needed
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed})")


class MemBuildError(_lib.LsmckError):
    """lsmck_memtable_build refused the batch: ``bad_index`` is the first
    invalid command (LSMCK_EINVAL), or ``needed`` the live entries' count when
    the array given holds fewer (LSMCK_ENOSPC); the other one is None."""

    def __init__(self, rc, what, bad_index=None, needed=None):
        self.bad_index = bad_index
        self.needed = needed
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed})")


class WritePlanError(_lib.LsmckError):
    """lsmck_db_write_plan refused the batch: ``bad_index`` is the first
    invalid command (LSMCK_EINVAL; None when the tombstone byte is missing or
    an argument is wrong), or ``needed`` = (entries, flushes) when an array
    given holds fewer (LSMCK_ENOSPC); the other one is None."""

    def __init__(self, rc, what, bad_index=None, needed=None):
        self.bad_index = bad_index
        self.needed = needed
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed})")


class ApplyPlanError(_lib.LsmckError):
    """lsmck_db_apply_plan refused the stream: ``bad_index`` is the first
    invalid command (LSMCK_EINVAL; None when the tombstone byte is missing or
    an argument is wrong), or ``needed`` = (entries, flushes, gets, misses)
    when an array given holds fewer (LSMCK_ENOSPC); the other one is None."""

    def __init__(self, rc, what, bad_index=None, needed=None):
        self.bad_index = bad_index
        self.needed = needed
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed})")


class SstDecodeError(_lib.LsmckError):
    """lsmck_sstable_decode_batch refused the batch: ``bad_index`` is the first
    table whose span is refused (LSMCK_EINVAL; None for an argument error), or
    ``needed`` the entries' count when the array given holds fewer
    (LSMCK_ENOSPC); the other one is None."""

    def __init__(self, rc, what, bad_index=None, needed=None):
        self.bad_index = bad_index
        self.needed = needed
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed})")


class SstMergeError(_lib.LsmckError):
    """lsmck_sstable_merge_batch refused the batch: ``bad_index`` is the first
    offending entry (LSMCK_EINVAL; None for an argument error) or, with
    ``stuck`` set, the first tombstone winner in (group, key) order
    (LSMCK_MERGE_STUCK: the reference's loop never terminates there);
    ``needed`` the winners' count when the array given holds fewer
    (LSMCK_ENOSPC)."""

    def __init__(self, rc, what, bad_index=None, needed=None, stuck=False):
        self.bad_index = bad_index
        self.needed = needed
        self.stuck = stuck
        super().__init__(rc, f"{what} (bad_index={bad_index}, needed={needed}, stuck={stuck})")


class SstGetError(_lib.LsmckError):
    """lsmck_sstable_get_batch refused the batch: ``bad_table`` is the first
    table whose span or index is refused, else ``bad_query`` the first query
    whose key range or reserved word is (LSMCK_EINVAL; both None for an
    argument error)."""

    def __init__(self, rc, what, bad_table=None, bad_query=None):
        self.bad_table = bad_table
        self.bad_query = bad_query
        super().__init__(rc, f"{what} (bad_table={bad_table}, bad_query={bad_query})")


class DbGetError(_lib.LsmckError):
    """lsmck_db_get_batch refused the batch: ``bad_run_entry`` is the first
    offending run entry, counted across the runs, else ``bad_table`` the first
    table refused, else ``bad_query`` the first query refused (LSMCK_EINVAL;
    all None for an argument error); or ``needed`` the gathered values' bytes
    when ``out`` holds fewer (LSMCK_ENOSPC)."""

    def __init__(self, rc, what, bad_run_entry=None, bad_table=None, bad_query=None, needed=None):
        self.bad_run_entry = bad_run_entry
        self.bad_table = bad_table
        self.bad_query = bad_query
        self.needed = needed
        super().__init__(rc, f"{what} (bad_run_entry={bad_run_entry}, bad_table={bad_table}, bad_query={bad_query}, "
                             f"needed={needed})")


class TableSet:
    """An opened table set (lsmck_tableset_open): ``Context.tableset_open``
    makes one.  It holds its context, so the context outlives it; ``close()``
    (or leaving the ``with`` block) frees the device buffers it owns."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def close(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.lsmck_tableset_close(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stat(self, key):
        """lsmck_tableset_stat: "tables", "items", "fenced_low", "fenced_high",
        "resident_bytes", and of a set opened with "bloom_bits" > 0 "bloom_tables",
        "bloom_keys" and "bloom_bytes" (0 otherwise)."""
        v = C.c_long()
        _lib.check(self.ctx.lib.lsmck_tableset_stat(self.handle, key.encode(), C.byref(v)), f"tableset_stat({key})")
        return v.value

    def _get(self, ctx, runs, qkeys, qb, q, n, res, out, out_cap, out_off, flags):
        none = 2 ** 64 - 1
        runs = np.ascontiguousarray(runs, dtype=_lib.GET_RUN_DTYPE)
        br, bq, nbytes = C.c_uint64(none), C.c_uint64(none), C.c_uint64(0)
        rc = ctx.lib.lsmck_tableset_get_batch(ctx.handle, self.handle, runs.ctypes.data if len(runs) else None, len(runs),
                                              qkeys, qb, q, n, res, out, out_cap, out_off, C.byref(nbytes), C.byref(br),
                                              C.byref(bq), flags)
        if rc == _lib.EINVAL:
            raise DbGetError(rc, "tableset_get_batch", bad_run_entry=None if br.value == none else br.value,
                             bad_query=None if bq.value == none else bq.value)
        if rc == _lib.ENOSPC:
            raise DbGetError(rc, "tableset_get_batch", needed=nbytes.value)
        _lib.check(rc, "tableset_get_batch")
        return nbytes.value

    def get_batch(self, runs, qkeys, queries, values=True, pinned=False, out_guess=1 << 20):
        """lsmck_tableset_get_batch, host form: ``Context.db_get_batch`` with
        the set in place of (data, index, spans); the same three results,
        ``val_off`` of a table's answer into the data arena the set was opened
        over.  Raises DbGetError."""
        keep, desc = [], np.zeros(len(runs), dtype=_lib.GET_RUN_DTYPE)
        for r, (keys, vals, ents) in enumerate(runs):
            keys = np.ascontiguousarray(keys, dtype=np.uint8)
            vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
            ents = np.ascontiguousarray(ents, dtype=_lib.WAL_CMD_DTYPE)
            keep.append((keys, vals, ents))
            desc[r] = (keys.ctypes.data if keys.nbytes else 0, keys.nbytes, vals.ctypes.data if vals.nbytes else 0,
                       vals.nbytes, ents.ctypes.data if len(ents) else 0, len(ents))
        qkeys = np.ascontiguousarray(qkeys, dtype=np.uint8)
        queries = np.ascontiguousarray(queries, dtype=_lib.GET_QUERY_DTYPE)
        n = len(queries)
        res = np.empty(n, dtype=_lib.GET_RESULT_DTYPE)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        args = (self.ctx, desc, _p(qkeys), qkeys.nbytes, _p(queries), n, _p(res))
        if not values:
            self._get(*args, None, 0, None, flags)
            return res, None, None
        off = np.empty(n + 1, dtype=np.uint64)
        out = np.empty(max(out_guess, 1), dtype=np.uint8)  # (a guess: the call names the size when it is too small)
        try:
            total = self._get(*args, _p(out), out.nbytes, off.ctypes.data, flags)
        except DbGetError as e:
            if e.needed is None:
                raise
            out = np.empty(e.needed, dtype=np.uint8)
            total = self._get(*args, _p(out), out.nbytes, off.ctypes.data, flags)
        return res, off, out[:total]

    def get_batch_device(self, runs, qkeys_ptr, qkeys_bytes, queries_ptr, n, res_ptr, out_ptr=None, out_cap=0,
                         out_off_ptr=None, ctx=None):
        """lsmck_tableset_get_batch on device pointers: ``runs`` and the
        outputs as in ``Context.db_get_batch_device``.  ``ctx``: the calling
        context (the set's own; another one is refused).  Returns the
        gathered bytes; raises DbGetError; nothing was written then."""
        if not isinstance(runs, np.ndarray):
            desc = np.zeros(len(runs), dtype=_lib.GET_RUN_DTYPE)
            for r, run in enumerate(runs):
                if hasattr(run, "image_bytes"):
                    run = (run.image.ptr, run.image_bytes, run.image.ptr, run.image_bytes, run.ents.ptr, run.nent)
                desc[r] = tuple(0 if x is None else int(x) for x in run)
            runs = desc
        return self._get(self.ctx if ctx is None else ctx, runs, qkeys_ptr, qkeys_bytes, queries_ptr, n, res_ptr, out_ptr,
                         out_cap, out_off_ptr, _lib.DEVICE)


class Context:
    def __init__(self, device=0):
        lib = _lib.load()
        self.lib = lib
        self.handle = lib.lsmck_ctx_create(device)
        if not self.handle:
            raise RuntimeError(f"lsmck_ctx_create({device}) failed: {_lib.last_error()}")
        self.device = device
        # records arrays of the last WAL replays per record dtype (pageable, page-locked),
        # reused once nothing refers to them
        self._wal_recs = {}
        self._wal_pinned = {}

    def _wal_recs_buffer(self, cap, dtype=None):
        """An uninitialised record array (WAL_REC_DTYPE, or WAL_REC16_DTYPE) of
        at least cap entries: the last replay's array again when no result
        refers to it any more (its pages are already mapped: a fresh worst-case
        n/9-entry array cost ~1 ms per 0.24 GB replay in allocation,
        first-touch faults and unmapping), else a new one."""
        dtype = WAL_REC_DTYPE if dtype is None else dtype
        buf = self._wal_recs.get(dtype.str)
        # references: the dict's, `buf`, getrefcount's argument -- any more is
        # a returned view still alive
        if buf is not None and len(buf) >= cap and sys.getrefcount(buf) <= 3:
            return buf
        buf = np.empty(cap, dtype=dtype)  # uninitialised: no zeroing of every slot
        self._wal_recs[dtype.str] = buf
        return buf

    def _wal_recs_pinned(self, cap, dtype=None):
        """A page-locked record array of at least cap entries (grow-only,
        reused once no result refers to it): the replay DMAs the records into it
        (LSMCK_RECS_PINNED).  The array's base is a holder of its PinnedBuffer,
        so the pinned memory lives as long as any view of it."""
        dtype = WAL_REC_DTYPE if dtype is None else dtype
        arr = self._wal_pinned.get(dtype.str)
        if arr is not None and len(arr) >= cap and sys.getrefcount(arr) <= 3:
            return arr
        arr = np.asarray(_PinnedRecords(PinnedBuffer(self, max(1, cap) * dtype.itemsize), max(1, cap), dtype))
        self._wal_pinned[dtype.str] = arr
        return arr

    def close(self):
        self._wal_pinned = {}
        if self.handle:
            self.lib.lsmck_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        _lib.check(self.lib.lsmck_ctx_set_option(self.handle, key.encode(), int(value)), f"set_option({key})")

    def get_stat(self, key):
        v = C.c_long()
        _lib.check(self.lib.lsmck_ctx_get_stat(self.handle, key.encode(), C.byref(v)), f"get_stat({key})")
        return v.value

    # --- memory -------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def alloc_pinned(self, nbytes):
        return PinnedBuffer(self, nbytes)

    def memcpy_d2h(self, dst_ptr, src_ptr, nbytes, stream=None):
        _lib.check(self.lib.lsmck_memcpy_d2h(self.handle, dst_ptr, src_ptr, nbytes, stream), "d2h")

    def sync(self, stream=None):
        _lib.check(self.lib.lsmck_stream_sync(self.handle, stream), "sync")

    def memset(self, ptr, value, nbytes, stream=None):
        _lib.check(self.lib.lsmck_memset_dev(self.handle, ptr, value, nbytes, stream), "memset")

    def gen_stream(self, dst_ptr, seed, byte_off, nbytes, stream=None):
        _lib.check(self.lib.lsmck_gen_stream(self.handle, dst_ptr, seed, byte_off, nbytes, stream), "gen_stream")

    # --- CRC-32, host arrays ------------------------------------------------
    def crc32(self, data, off, length, pinned=False):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        n = len(off)
        out = np.empty(n, dtype=np.uint32)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        _lib.check(self.lib.lsmck_crc32_batch(self.handle, data.ctypes.data, off.ctypes.data, length.ctypes.data, n,
                                              out.ctypes.data, flags, None), "crc32_batch")
        return out

    def crc32_fixed(self, data, stride, length, n, pinned=False):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.empty(n, dtype=np.uint32)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        _lib.check(self.lib.lsmck_crc32_batch_fixed(self.handle, data.ctypes.data, stride, length, n, out.ctypes.data,
                                                    flags, None), "crc32_batch_fixed")
        return out

    def crc32_verify(self, data, off, length, expected):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        expected = np.ascontiguousarray(expected, dtype=np.uint32)
        nb, fb = C.c_uint64(), C.c_uint64()
        rc = _lib.check(self.lib.lsmck_crc32_verify_batch(self.handle, data.ctypes.data, off.ctypes.data,
                                                          length.ctypes.data, expected.ctypes.data, len(off),
                                                          _lib.HOST, None, C.byref(nb), C.byref(fb)), "verify")
        return rc, nb.value, fb.value

    # --- CRC-32, device pointers (async on stream) ----------------------------
    def crc32_device(self, base, off, length, n, out, stream=None, sorted_span=False):
        """sorted_span: LSMCK_SORTED, the caller asserts its records are sorted inside one readable span"""
        flags = _lib.DEVICE | (_lib.SORTED if sorted_span else 0)
        _lib.check(self.lib.lsmck_crc32_batch(self.handle, base, off, length, n, out, flags, stream),
                   "crc32_batch(device)")

    def crc32_fixed_device(self, base, stride, length, n, out, stream=None):
        _lib.check(self.lib.lsmck_crc32_batch_fixed(self.handle, base, stride, length, n, out, _lib.DEVICE, stream),
                   "crc32_batch_fixed(device)")

    def crc32_verify_device(self, base, off, length, expected, n, stream=None):
        nb, fb = C.c_uint64(), C.c_uint64()
        rc = _lib.check(self.lib.lsmck_crc32_verify_batch(self.handle, base, off, length, expected, n, _lib.DEVICE,
                                                          stream, C.byref(nb), C.byref(fb)), "verify(device)")
        return rc, nb.value, fb.value

    # --- SHA-256 --------------------------------------------------------------
    def sha256(self, data, off, length, pinned=False):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        n = len(off)
        out = np.empty((n, 32), dtype=np.uint8)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        _lib.check(self.lib.lsmck_sha256_batch(self.handle, data.ctypes.data, off.ctypes.data, length.ctypes.data, n,
                                               out.ctypes.data, flags, None), "sha256_batch")
        return out

    def sha256_fixed(self, data, stride, length, n, pinned=False):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.empty((n, 32), dtype=np.uint8)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        _lib.check(self.lib.lsmck_sha256_batch_fixed(self.handle, data.ctypes.data, stride, length, n,
                                                     out.ctypes.data, flags, None), "sha256_batch_fixed")
        return out

    def sha256_device(self, base, off, length, n, out, stream=None):
        _lib.check(self.lib.lsmck_sha256_batch(self.handle, base, off, length, n, out, _lib.DEVICE, stream),
                   "sha256_batch(device)")

    def sha256_fixed_device(self, base, stride, length, n, out, stream=None):
        _lib.check(self.lib.lsmck_sha256_batch_fixed(self.handle, base, stride, length, n, out, _lib.DEVICE, stream),
                   "sha256_batch_fixed(device)")

    # --- WAL / SSTable batch verify ---------------------------------------------
    def wal_frame_insert_device(self, img_ptr, off_ptr, len_ptr, crc_ptr, n, kmax=16, stream=None):
        """lsmck_wal_frame_insert_device: Insert headers in front of n payloads
        of a device-resident log (all device pointers)."""
        _lib.check(self.lib.lsmck_wal_frame_insert_device(self.handle, img_ptr, off_ptr, len_ptr, crc_ptr, n, kmax,
                                                           stream), "wal_frame_insert_device")

    def _wal_encode(self, keys, kb, vals, vb, cmds, n, img, cap, rec_off, flags):
        none = 2 ** 64 - 1
        nbytes, bad = C.c_size_t(), C.c_uint64(none)
        rc = self.lib.lsmck_wal_encode_batch(self.handle, keys, kb, vals, vb, cmds, n, img, cap, C.byref(nbytes),
                                             rec_off, C.byref(bad), flags)
        if rc == _lib.EINVAL and bad.value != none:
            raise WalEncodeError(rc, "wal_encode_batch", bad_index=bad.value)
        if rc == _lib.ENOSPC:
            raise WalEncodeError(rc, "wal_encode_batch", needed=nbytes.value)
        _lib.check(rc, "wal_encode_batch")
        return nbytes.value

    def wal_encode_batch(self, keys, vals, cmds, pinned=False):
        """lsmck_wal_encode_batch, host form: the log image of the commands
        ``cmds`` (WAL_CMD_DTYPE: key / value ranges in the uint8 arenas
        ``keys`` / ``vals``, which may be one array), encoded on the GPU.
        Returns (image: np.uint8 array, rec_off: np.uint64 array of the
        records' header offsets).  Raises WalEncodeError (``bad_index``: the
        first invalid command)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        cmds = np.ascontiguousarray(cmds, dtype=_lib.WAL_CMD_DTYPE)
        n = len(cmds)
        size = self.lib.lsmck_wal_encoded_size(cmds.ctypes.data, n)
        if size == 2 ** 64 - 1:
            size = 0  # (the call reports the first invalid command)
        img = np.empty(size, dtype=np.uint8)
        rec_off = np.empty(n, dtype=np.uint64)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        got = self._wal_encode(keys.ctypes.data, keys.nbytes, vals.ctypes.data, vals.nbytes, cmds.ctypes.data, n,
                               img.ctypes.data, size, rec_off.ctypes.data, flags)
        assert got == size
        return img, rec_off

    def wal_encode_batch_device(self, keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, img_ptr, cap,
                                rec_off_ptr=None):
        """lsmck_wal_encode_batch on device pointers (cmds: n lsmck_wal_cmd;
        rec_off_ptr: n u64 or None).  Returns the image's bytes; raises
        WalEncodeError with ``bad_index`` (an invalid command) or ``needed``
        (cap is smaller than the encoded size); nothing was written then."""
        return self._wal_encode(keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, img_ptr, cap, rec_off_ptr,
                                _lib.DEVICE)

    def _sst_encode(self, keys, kb, vals, vb, ents, n, table_first, data, data_cap, index, index_cap, spans,
                    data_sha, index_sha, flags):
        none = 2 ** 64 - 1
        tf = np.ascontiguousarray(table_first, dtype=np.uint64)
        if len(tf) < 1:
            raise ValueError("table_first holds ntab + 1 values")
        db, ib, bad = C.c_size_t(), C.c_size_t(), C.c_uint64(none)
        rc = self.lib.lsmck_sstable_encode_batch(self.handle, keys, kb, vals, vb, ents, n, tf.ctypes.data, len(tf) - 1,
                                                 data, data_cap, index, index_cap, spans, data_sha, index_sha,
                                                 C.byref(db), C.byref(ib), C.byref(bad), flags)
        if rc == _lib.EINVAL:
            raise SstEncodeError(rc, "sstable_encode_batch", bad_index=None if bad.value == none else bad.value)
        if rc == _lib.ENOSPC:
            raise SstEncodeError(rc, "sstable_encode_batch", needed=(db.value, ib.value))
        _lib.check(rc, "sstable_encode_batch")
        return db.value, ib.value

    def sstable_encode_batch(self, keys, vals, ents, table_first, digests=True, pinned=False):
        """lsmck_sstable_encode_batch, host form: the data and index files of
        the tables that ``table_first`` (ntab + 1 entry indices) cuts the
        entries ``ents`` (WAL_CMD_DTYPE, type 1: key / value ranges in the
        uint8 arenas ``keys`` / ``vals``, which may be one array) into,
        encoded and hashed on the GPU.  Returns (data, index: np.uint8 arrays,
        the tables' files back to back; spans: SSTABLE_SPAN_DTYPE per table;
        data_sha, index_sha: (ntab, 32) uint8, or None without ``digests``).
        Raises SstEncodeError (``bad_index``: the first offending entry)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        ents = np.ascontiguousarray(ents, dtype=_lib.WAL_CMD_DTYPE)
        tf = np.ascontiguousarray(table_first, dtype=np.uint64)
        n, ntab = len(ents), len(tf) - 1
        db, ib = C.c_uint64(), C.c_uint64()
        if self.lib.lsmck_sstable_encoded_size(ents.ctypes.data, n, tf.ctypes.data, ntab, C.byref(db), C.byref(ib)):
            db, ib = C.c_uint64(0), C.c_uint64(0)  # (the call reports what is wrong)
        data, index = np.empty(db.value, dtype=np.uint8), np.empty(ib.value, dtype=np.uint8)
        spans = np.empty(ntab, dtype=_lib.SSTABLE_SPAN_DTYPE)
        dsha = np.empty((ntab, 32), dtype=np.uint8) if digests else None
        isha = np.empty((ntab, 32), dtype=np.uint8) if digests else None
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        got = self._sst_encode(keys.ctypes.data, keys.nbytes, vals.ctypes.data, vals.nbytes, ents.ctypes.data, n, tf,
                               data.ctypes.data, data.nbytes, index.ctypes.data, index.nbytes, spans.ctypes.data,
                               _p(dsha), _p(isha), flags)
        assert got == (db.value, ib.value)
        return data, index, spans, dsha, isha

    def sstable_encode_batch_device(self, keys_ptr, keys_bytes, vals_ptr, vals_bytes, ents_ptr, n, table_first,
                                    data_ptr, data_cap, index_ptr, index_cap, spans_ptr=None, data_sha_ptr=None,
                                    index_sha_ptr=None):
        """lsmck_sstable_encode_batch on device pointers (ents: n lsmck_wal_cmd;
        table_first: a host array of ntab + 1 values; spans_ptr: ntab
        lsmck_sstable_span or None; the digest pointers: 32 * ntab bytes each
        or None -- that image is not hashed).  Returns (data_bytes,
        index_bytes); raises SstEncodeError with ``bad_index`` or ``needed``;
        nothing was written then."""
        return self._sst_encode(keys_ptr, keys_bytes, vals_ptr, vals_bytes, ents_ptr, n, table_first, data_ptr,
                                data_cap, index_ptr, index_cap, spans_ptr, data_sha_ptr, index_sha_ptr, _lib.DEVICE)

    def _mem_build(self, keys, kb, vals, vb, cmds, n, ents, cap, src, flags):
        none = 2 ** 64 - 1
        nent, nbytes, bad = C.c_size_t(), C.c_uint64(), C.c_uint64(none)
        rc = self.lib.lsmck_memtable_build(self.handle, keys, kb, vals, vb, cmds, n, ents, cap, src, C.byref(nent),
                                           C.byref(nbytes), C.byref(bad), flags)
        if rc == _lib.EINVAL and bad.value != none:
            raise MemBuildError(rc, "memtable_build", bad_index=bad.value)
        if rc == _lib.ENOSPC:
            raise MemBuildError(rc, "memtable_build", needed=nent.value)
        _lib.check(rc, "memtable_build")
        return nent.value, nbytes.value

    def memtable_build(self, keys, vals, cmds, pinned=False):
        """lsmck_memtable_build, host form: the memtable of the commands
        ``cmds`` (WAL_CMD_DTYPE in log order: key / value ranges in the uint8
        arenas ``keys`` / ``vals``, which may be one array), sorted and
        resolved on the GPU.  Returns (ents: WAL_CMD_DTYPE, the live entries
        in key order, their ranges in the same arenas; src: np.uint32, the
        command each came from; mem_bytes: the reference's size_in_bytes()).
        Raises MemBuildError (``bad_index``: the first invalid command)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        cmds = np.ascontiguousarray(cmds, dtype=_lib.WAL_CMD_DTYPE)
        n = len(cmds)
        ents = np.empty(n, dtype=_lib.WAL_CMD_DTYPE)  # (at most every command is live)
        src = np.empty(n, dtype=np.uint32)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        nent, nbytes = self._mem_build(keys.ctypes.data, keys.nbytes, vals.ctypes.data, vals.nbytes, cmds.ctypes.data,
                                       n, ents.ctypes.data, n, src.ctypes.data, flags)
        return ents[:nent], src[:nent], nbytes

    def memtable_build_device(self, keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, ents_ptr, cap,
                              src_ptr=None):
        """lsmck_memtable_build on device pointers (cmds: n lsmck_wal_cmd;
        ents: cap lsmck_wal_cmd; src_ptr: cap u32 or None).  Returns (nent,
        mem_bytes); raises MemBuildError with ``bad_index`` (an invalid
        command) or ``needed`` (cap is smaller than the live entries' count);
        nothing was written then."""
        return self._mem_build(keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, ents_ptr, cap, src_ptr,
                               _lib.DEVICE)

    def _sst_decode(self, data, db, index, ib, spans, ntab, ents, cap, consumed, flags):
        none = 2 ** 64 - 1
        tf = np.zeros(ntab + 1, dtype=np.uint64)
        nent, bad = C.c_size_t(), C.c_uint64(none)
        rc = self.lib.lsmck_sstable_decode_batch(self.handle, data, db, index, ib, spans, ntab, ents, cap,
                                                 tf.ctypes.data, consumed, C.byref(nent), C.byref(bad), flags)
        if rc == _lib.EINVAL:
            raise SstDecodeError(rc, "sstable_decode_batch", bad_index=None if bad.value == none else bad.value)
        if rc == _lib.ENOSPC:
            raise SstDecodeError(rc, "sstable_decode_batch", needed=nent.value)
        _lib.check(rc, "sstable_decode_batch")
        return nent.value, tf

    def sstable_decode_batch(self, data, spans, index=None, pinned=False):
        """lsmck_sstable_decode_batch, host form: the entries of the tables
        whose data files lie in the uint8 arena ``data`` at ``spans``
        (SSTABLE_SPAN_DTYPE; ``index``: the arena of their index files, or
        None), walked on the GPU as the reference's iterator walks them.
        Returns (ents: WAL_CMD_DTYPE, key_off / val_off into ``data``;
        tab_first: np.uint64, ntab + 1; consumed: np.uint64 per table).
        Raises SstDecodeError (``bad_index``: the first table refused)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        index = None if index is None else np.ascontiguousarray(index, dtype=np.uint8)
        spans = np.ascontiguousarray(spans, dtype=_lib.SSTABLE_SPAN_DTYPE)
        ntab = len(spans)
        ents = np.empty(data.nbytes // 8, dtype=_lib.WAL_CMD_DTYPE)  # (a record is 8 bytes or more)
        consumed = np.zeros(ntab, dtype=np.uint64)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        try:
            nent, tf = self._sst_decode(data.ctypes.data, data.nbytes, _p(index), 0 if index is None else index.nbytes,
                                        spans.ctypes.data, ntab, ents.ctypes.data, len(ents), consumed.ctypes.data,
                                        flags)
        except SstDecodeError as e:
            if e.needed is None:
                raise
            ents = np.empty(e.needed, dtype=_lib.WAL_CMD_DTYPE)  # (overlapping spans: more entries than bytes / 8)
            nent, tf = self._sst_decode(data.ctypes.data, data.nbytes, _p(index), 0 if index is None else index.nbytes,
                                        spans.ctypes.data, ntab, ents.ctypes.data, len(ents), consumed.ctypes.data,
                                        flags)
        return ents[:nent], tf, consumed

    def sstable_decode_batch_device(self, data_ptr, data_bytes, index_ptr, index_bytes, spans_ptr, ntab, ents_ptr, cap,
                                    consumed_ptr=None):
        """lsmck_sstable_decode_batch on device pointers (spans: ntab
        lsmck_sstable_span; index_ptr: None without a hint; ents: cap
        lsmck_wal_cmd; consumed_ptr: ntab u64 or None).  Returns (nent,
        tab_first: a host np.uint64 array of ntab + 1); raises SstDecodeError
        with ``bad_index`` or ``needed``; nothing was written then."""
        return self._sst_decode(data_ptr, data_bytes, index_ptr, index_bytes, spans_ptr, ntab, ents_ptr, cap,
                                consumed_ptr, _lib.DEVICE)

    def _sst_merge(self, keys, kb, vals, vb, ents, n, tab_first, group_first, out, cap, src, flags, tombstones):
        none = 2 ** 64 - 1
        mode = {"stuck": 0, "drop": _lib.MERGE_DROP_TOMBSTONES, "keep": _lib.MERGE_KEEP_TOMBSTONES}[tombstones]
        tf = np.ascontiguousarray(tab_first, dtype=np.uint64)
        gf = np.ascontiguousarray(group_first, dtype=np.uint64)
        if len(tf) < 1 or len(gf) < 1:
            raise ValueError("tab_first holds ntab + 1 values, group_first ngrp + 1")
        of = np.zeros(len(gf), dtype=np.uint64)
        nout, bad = C.c_size_t(), C.c_uint64(none)
        rc = self.lib.lsmck_sstable_merge_batch(self.handle, keys, kb, vals, vb, ents, n, tf.ctypes.data, len(tf) - 1,
                                                gf.ctypes.data, len(gf) - 1, out, cap, src, of.ctypes.data,
                                                C.byref(nout), C.byref(bad), flags | mode)
        if rc == _lib.MERGE_STUCK:
            raise SstMergeError(rc, "sstable_merge_batch", bad_index=bad.value, stuck=True)
        if rc == _lib.EINVAL:
            raise SstMergeError(rc, "sstable_merge_batch", bad_index=None if bad.value == none else bad.value)
        if rc == _lib.ENOSPC:
            raise SstMergeError(rc, "sstable_merge_batch", needed=nout.value)
        _lib.check(rc, "sstable_merge_batch")
        return nout.value, of

    def sstable_merge_batch(self, keys, vals, ents, tab_first, group_first, tombstones="stuck", pinned=False):
        """lsmck_sstable_merge_batch, host form: the sorted tables that
        ``tab_first`` cuts ``ents`` into, merged group by group
        (``group_first``: ngrp + 1 table numbers; oldest table first, the
        newest wins a key) on the GPU.  ``tombstones``: "stuck" (a tombstone
        winner raises SstMergeError with ``stuck``), "drop" or "keep".
        Returns (out: WAL_CMD_DTYPE, the winners in key order, group after
        group; src: np.uint32, their indices in ``ents``; out_first:
        np.uint64, ngrp + 1)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        ents = np.ascontiguousarray(ents, dtype=_lib.WAL_CMD_DTYPE)
        n = len(ents)
        out = np.empty(n, dtype=_lib.WAL_CMD_DTYPE)  # (at most every entry wins)
        src = np.empty(n, dtype=np.uint32)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        nout, of = self._sst_merge(keys.ctypes.data, keys.nbytes, vals.ctypes.data, vals.nbytes, ents.ctypes.data, n,
                                   tab_first, group_first, out.ctypes.data, n, src.ctypes.data, flags, tombstones)
        return out[:nout], src[:nout], of

    def sstable_merge_batch_device(self, keys_ptr, keys_bytes, vals_ptr, vals_bytes, ents_ptr, n, tab_first,
                                   group_first, out_ptr, cap, src_ptr=None, tombstones="stuck"):
        """lsmck_sstable_merge_batch on device pointers (ents: n lsmck_wal_cmd;
        tab_first, group_first: host arrays; out: cap lsmck_wal_cmd; src_ptr:
        cap u32 or None).  Returns (nout, out_first: a host np.uint64 array of
        ngrp + 1); raises SstMergeError; nothing was written then."""
        return self._sst_merge(keys_ptr, keys_bytes, vals_ptr, vals_bytes, ents_ptr, n, tab_first, group_first, out_ptr,
                               cap, src_ptr, _lib.DEVICE, tombstones)

    def _sst_get(self, data, db, index, ib, spans, ntab, qkeys, qb, q, n, res, flags):
        none = 2 ** 64 - 1
        bt, bq = C.c_uint64(none), C.c_uint64(none)
        rc = self.lib.lsmck_sstable_get_batch(self.handle, data, db, index, ib, spans, ntab, qkeys, qb, q, n, res,
                                              C.byref(bt), C.byref(bq), flags)
        if rc == _lib.EINVAL:
            raise SstGetError(rc, "sstable_get_batch", bad_table=None if bt.value == none else bt.value,
                              bad_query=None if bq.value == none else bq.value)
        _lib.check(rc, "sstable_get_batch")

    def sstable_get_batch(self, data, index, spans, qkeys, queries, pinned=False):
        """lsmck_sstable_get_batch, host form: SsTable::get of every query
        (GET_QUERY_DTYPE: key ranges in the uint8 arena ``qkeys``) over the
        tables whose data and index files lie in the uint8 arenas ``data`` and
        ``index`` at ``spans`` (SSTABLE_SPAN_DTYPE, in search order), the first
        table that answers winning.  Returns GET_RESULT_DTYPE per query:
        ``table`` (GET_NONE: no table answered), ``val_off`` into ``data``
        (bit 63, GET_TOMBSTONE: the value is the byte 0) and ``vlen``.  Raises
        SstGetError (``bad_table`` or ``bad_query``)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        index = np.ascontiguousarray(index, dtype=np.uint8)
        spans = np.ascontiguousarray(spans, dtype=_lib.SSTABLE_SPAN_DTYPE)
        qkeys = np.ascontiguousarray(qkeys, dtype=np.uint8)
        queries = np.ascontiguousarray(queries, dtype=_lib.GET_QUERY_DTYPE)
        res = np.empty(len(queries), dtype=_lib.GET_RESULT_DTYPE)
        self._sst_get(data.ctypes.data, data.nbytes, index.ctypes.data, index.nbytes, spans.ctypes.data, len(spans),
                      qkeys.ctypes.data, qkeys.nbytes, queries.ctypes.data, len(queries), res.ctypes.data,
                      _lib.HOST_PINNED if pinned else _lib.HOST)
        return res

    def sstable_get_batch_device(self, data_ptr, data_bytes, index_ptr, index_bytes, spans_ptr, ntab, qkeys_ptr,
                                 qkeys_bytes, queries_ptr, n, res_ptr):
        """lsmck_sstable_get_batch on device pointers (spans: ntab
        lsmck_sstable_span; queries: n lsmck_get_query, 8-byte aligned; res: n
        lsmck_get_result).  Raises SstGetError; nothing was written then."""
        self._sst_get(data_ptr, data_bytes, index_ptr, index_bytes, spans_ptr, ntab, qkeys_ptr, qkeys_bytes, queries_ptr,
                      n, res_ptr, _lib.DEVICE)

    def _db_get(self, runs, data, db, index, ib, spans, ntab, qkeys, qb, q, n, res, out, out_cap, out_off, flags):
        none = 2 ** 64 - 1
        runs = np.ascontiguousarray(runs, dtype=_lib.GET_RUN_DTYPE)
        br, bt, bq, nbytes = C.c_uint64(none), C.c_uint64(none), C.c_uint64(none), C.c_uint64(0)
        rc = self.lib.lsmck_db_get_batch(self.handle, runs.ctypes.data if len(runs) else None, len(runs), data, db,
                                         index, ib, spans, ntab, qkeys, qb, q, n, res, out, out_cap, out_off,
                                         C.byref(nbytes), C.byref(br), C.byref(bt), C.byref(bq), flags)
        if rc == _lib.EINVAL:
            raise DbGetError(rc, "db_get_batch", *(None if w.value == none else w.value for w in (br, bt, bq)))
        if rc == _lib.ENOSPC:
            raise DbGetError(rc, "db_get_batch", needed=nbytes.value)
        _lib.check(rc, "db_get_batch")
        return nbytes.value

    def db_get_batch(self, runs, data, index, spans, qkeys, queries, values=True, pinned=False):
        """lsmck_db_get_batch, host form: Db::get of every query
        (GET_QUERY_DTYPE over the uint8 arena ``qkeys``) over ``runs`` -- a
        list of (keys, vals, ents): two uint8 arenas, which may be one array,
        and WAL_CMD_DTYPE entries in strictly increasing key order; the
        memtable first, then the old one -- and then the tables of
        ``sstable_get_batch``.  Returns (res, out_off, out): GET_RESULT_DTYPE
        per query (``table``: the source number, the runs first; ``val_off``
        into the winning run's vals or ``data``), and with ``values`` the
        exclusive scan of the answered lengths (np.uint64, n + 1) and the
        values packed in that order (np.uint8) -- a tombstone or a miss has no
        byte; both None without.  Raises DbGetError."""
        keep, desc = [], np.zeros(len(runs), dtype=_lib.GET_RUN_DTYPE)
        for r, (keys, vals, ents) in enumerate(runs):
            keys = np.ascontiguousarray(keys, dtype=np.uint8)
            vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
            ents = np.ascontiguousarray(ents, dtype=_lib.WAL_CMD_DTYPE)
            keep.append((keys, vals, ents))
            desc[r] = (keys.ctypes.data if keys.nbytes else 0, keys.nbytes, vals.ctypes.data if vals.nbytes else 0,
                       vals.nbytes, ents.ctypes.data if len(ents) else 0, len(ents))
        data = np.ascontiguousarray(data, dtype=np.uint8)
        index = np.ascontiguousarray(index, dtype=np.uint8)
        spans = np.ascontiguousarray(spans, dtype=_lib.SSTABLE_SPAN_DTYPE)
        qkeys = np.ascontiguousarray(qkeys, dtype=np.uint8)
        queries = np.ascontiguousarray(queries, dtype=_lib.GET_QUERY_DTYPE)
        n = len(queries)
        res = np.empty(n, dtype=_lib.GET_RESULT_DTYPE)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        args = (desc, _p(data), data.nbytes, _p(index), index.nbytes, _p(spans), len(spans), _p(qkeys), qkeys.nbytes,
                _p(queries), n, _p(res))
        if not values:
            self._db_get(*args, None, 0, None, flags)
            return res, None, None
        off = np.empty(n + 1, dtype=np.uint64)
        # a value is at most its source's bytes; a key asked twice is gathered twice, so the first size is a guess
        out = np.empty(min(data.nbytes + sum(v.nbytes for _, v, _ in keep), 1 << 20), dtype=np.uint8)
        try:
            total = self._db_get(*args, _p(out), out.nbytes, off.ctypes.data, flags)
        except DbGetError as e:
            if e.needed is None:
                raise
            out = np.empty(e.needed, dtype=np.uint8)
            total = self._db_get(*args, _p(out), out.nbytes, off.ctypes.data, flags)
        return res, off, out[:total]

    def db_get_batch_device(self, runs, data_ptr, data_bytes, index_ptr, index_bytes, spans_ptr, ntab, qkeys_ptr,
                            qkeys_bytes, queries_ptr, n, res_ptr, out_ptr=None, out_cap=0, out_off_ptr=None):
        """lsmck_db_get_batch on device pointers.  ``runs``: GET_RUN_DTYPE (a
        host array of device pointers and sizes), or a list whose items are
        such tuples (keys_ptr, keys_bytes, vals_ptr, vals_bytes, ents_ptr,
        nent) or ``wal.DeviceMemTable``s (the image is both arenas).
        ``out_off_ptr``: n + 1 u64 for the gather, or None for the results
        alone.  Returns the gathered bytes; raises DbGetError (``needed``: the
        bytes when out_cap is smaller); nothing was written then."""
        if not isinstance(runs, np.ndarray):
            desc = np.zeros(len(runs), dtype=_lib.GET_RUN_DTYPE)
            for r, run in enumerate(runs):
                if hasattr(run, "image_bytes"):
                    run = (run.image.ptr, run.image_bytes, run.image.ptr, run.image_bytes, run.ents.ptr, run.nent)
                desc[r] = tuple(0 if x is None else int(x) for x in run)
            runs = desc
        return self._db_get(runs, data_ptr, data_bytes, index_ptr, index_bytes, spans_ptr, ntab, qkeys_ptr, qkeys_bytes,
                            queries_ptr, n, res_ptr, out_ptr, out_cap, out_off_ptr, _lib.DEVICE)

    def tableset_open(self, data, index, spans, ntab=None, data_bytes=None, index_bytes=None, pinned=False):
        """lsmck_tableset_open: the tables of ``sstable_get_batch`` opened once
        -- the index pass and the key fences stay on the device.  Host form:
        ``data`` and ``index`` uint8 arrays, ``spans`` SSTABLE_SPAN_DTYPE; the
        set owns device copies.  Device form (``ntab`` given): three device
        pointers with ``data_bytes`` and ``index_bytes``; the set borrows data
        and index, which stay alive and unchanged until it is closed.  Returns
        a ``TableSet``; raises SstGetError (``bad_table``)."""
        if ntab is None:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            index = np.ascontiguousarray(index, dtype=np.uint8)
            spans = np.ascontiguousarray(spans, dtype=_lib.SSTABLE_SPAN_DTYPE)
            args = (_p(data), data.nbytes, _p(index), index.nbytes, _p(spans), len(spans))
            flags = _lib.HOST_PINNED if pinned else _lib.HOST
        else:
            args, flags = (data, data_bytes, index, index_bytes, spans, ntab), _lib.DEVICE
        none = 2 ** 64 - 1
        handle, bt = C.c_void_p(), C.c_uint64(none)
        rc = self.lib.lsmck_tableset_open(self.handle, *args, C.byref(handle), C.byref(bt), flags)
        if rc == _lib.EINVAL:
            raise SstGetError(rc, "tableset_open", bad_table=None if bt.value == none else bt.value)
        _lib.check(rc, "tableset_open")
        return TableSet(self, handle.value)

    def _write_plan(self, keys, kb, vals, vb, cmds, n, limit, tomb_off, ents, ent_cap, src, segs, seg_cap, flags):
        none = 2 ** 64 - 1
        nent, nflush, bad = C.c_size_t(), C.c_size_t(), C.c_uint64(none)
        rc = self.lib.lsmck_db_write_plan(self.handle, keys, kb, vals, vb, cmds, n, limit, tomb_off, ents, ent_cap, src,
                                          segs, seg_cap, C.byref(nent), C.byref(nflush), C.byref(bad), flags)
        if rc == _lib.EINVAL:
            raise WritePlanError(rc, "db_write_plan", bad_index=None if bad.value == none else bad.value)
        if rc == _lib.ENOSPC:
            raise WritePlanError(rc, "db_write_plan", needed=(nent.value, nflush.value))
        _lib.check(rc, "db_write_plan")
        return nent.value, nflush.value

    def db_write_plan(self, keys, vals, cmds, limit, tomb_off, pinned=False):
        """lsmck_db_write_plan, host form: where the command stream ``cmds``
        (WAL_CMD_DTYPE in order, type 1 Insert / 2 delete: key / value ranges
        in the uint8 arenas ``keys`` / ``vals``) flushes at ``limit`` bytes,
        and every memtable's entries.  ``vals[tomb_off]`` is the 0 byte a
        delete's entry points at.  Returns (ents: WAL_CMD_DTYPE, segment after
        segment in key order; src: np.uint32, the command each came from;
        segs: WRITE_SEG_DTYPE, nflush + 1 items, the last one the memtable
        left).  Raises WritePlanError (``bad_index``: the first invalid
        command, None for the tombstone byte)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        cmds = np.ascontiguousarray(cmds, dtype=_lib.WAL_CMD_DTYPE)
        n = len(cmds)
        ents = np.empty(n, dtype=_lib.WAL_CMD_DTYPE)  # (at most every command is an entry, and closes a segment)
        src = np.empty(n, dtype=np.uint32)
        segs = np.empty(n + 1, dtype=_lib.WRITE_SEG_DTYPE)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        nent, nflush = self._write_plan(_p(keys), keys.nbytes, _p(vals), vals.nbytes, _p(cmds), n, limit, tomb_off,
                                        ents.ctypes.data, n, src.ctypes.data, segs.ctypes.data, n + 1, flags)
        return ents[:nent], src[:nent], segs[:nflush + 1]

    def db_write_plan_device(self, keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, limit, tomb_off, ents_ptr,
                             ent_cap, src_ptr, segs_ptr, seg_cap):
        """lsmck_db_write_plan on device pointers (cmds: n lsmck_wal_cmd; ents:
        ent_cap lsmck_wal_cmd; src_ptr: ent_cap u32 or None; segs: seg_cap
        lsmck_write_seg).  Returns (nent, nflush); raises WritePlanError with
        ``bad_index`` or ``needed`` = (the entries, the flushes: one segment
        fewer than segs must hold); nothing was written then."""
        return self._write_plan(keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, limit, tomb_off, ents_ptr,
                                ent_cap, src_ptr, segs_ptr, seg_cap, _lib.DEVICE)

    def _apply_plan(self, keys, kb, vals, vb, cmds, n, limit, tomb_off, ents, ent_cap, src, segs, seg_cap, gets,
                    get_cap, miss_q, miss_get, flags):
        none = 2 ** 64 - 1
        nent, nflush, nget, nmiss, bad = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_uint64(none)
        rc = self.lib.lsmck_db_apply_plan(self.handle, keys, kb, vals, vb, cmds, n, limit, tomb_off, ents, ent_cap, src,
                                          segs, seg_cap, gets, get_cap, miss_q, miss_get, C.byref(nent),
                                          C.byref(nflush), C.byref(nget), C.byref(nmiss), C.byref(bad), flags)
        if rc == _lib.EINVAL:
            raise ApplyPlanError(rc, "db_apply_plan", bad_index=None if bad.value == none else bad.value)
        if rc == _lib.ENOSPC:
            raise ApplyPlanError(rc, "db_apply_plan", needed=(nent.value, nflush.value, nget.value, nmiss.value))
        _lib.check(rc, "db_apply_plan")
        return nent.value, nflush.value, nget.value, nmiss.value

    def db_apply_plan(self, keys, vals, cmds, limit, tomb_off, pinned=False):
        """lsmck_db_apply_plan, host form: ``db_write_plan`` over a stream
        that also holds Gets (type ``_lib.CMD_GET``), each answered by the
        last write in front of it.  Returns (ents, src, segs as
        ``db_write_plan`` does; gets: APPLY_GET_DTYPE, the Gets in stream
        order; miss_q: GET_QUERY_DTYPE over ``keys`` and miss_get: np.uint32,
        the Gets no write of the stream answers).  Raises ApplyPlanError."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        vals = keys if vals is keys else np.ascontiguousarray(vals, dtype=np.uint8)
        cmds = np.ascontiguousarray(cmds, dtype=_lib.WAL_CMD_DTYPE)
        n = len(cmds)
        ents = np.empty(n, dtype=_lib.WAL_CMD_DTYPE)
        src = np.empty(n, dtype=np.uint32)
        segs = np.empty(n + 1, dtype=_lib.WRITE_SEG_DTYPE)
        gets = np.empty(n, dtype=_lib.APPLY_GET_DTYPE)
        miss_q = np.empty(n, dtype=_lib.GET_QUERY_DTYPE)
        miss_get = np.empty(n, dtype=np.uint32)
        flags = _lib.HOST_PINNED if pinned else _lib.HOST
        nent, nflush, nget, nmiss = self._apply_plan(
            _p(keys), keys.nbytes, _p(vals), vals.nbytes, _p(cmds), n, limit, tomb_off, ents.ctypes.data, n,
            src.ctypes.data, segs.ctypes.data, n + 1, gets.ctypes.data, n, miss_q.ctypes.data, miss_get.ctypes.data,
            flags)
        return ents[:nent], src[:nent], segs[:nflush + 1], gets[:nget], miss_q[:nmiss], miss_get[:nmiss]

    def db_apply_plan_device(self, keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, limit, tomb_off, ents_ptr,
                             ent_cap, src_ptr, segs_ptr, seg_cap, gets_ptr, get_cap, miss_q_ptr=None,
                             miss_get_ptr=None):
        """lsmck_db_apply_plan on device pointers (as ``db_write_plan_device``;
        gets: get_cap lsmck_apply_get; miss_q / miss_get: get_cap
        lsmck_get_query / u32, both or neither).  Returns (nent, nflush, nget,
        nmiss); raises ApplyPlanError with ``bad_index`` or ``needed`` = the
        four counts; nothing was written then."""
        return self._apply_plan(keys_ptr, keys_bytes, vals_ptr, vals_bytes, cmds_ptr, n, limit, tomb_off, ents_ptr,
                                ent_cap, src_ptr, segs_ptr, seg_cap, gets_ptr, get_cap, miss_q_ptr, miss_get_ptr,
                                _lib.DEVICE)

    def wal_recs_to_cmds_device(self, recs_ptr, n, img_bytes, cmds_ptr, stream=None):
        """lsmck_wal_recs_to_cmds: n compact replay records (lsmck_wal_rec16,
        device) as lsmck_wal_cmd (device) over the log image of img_bytes
        bytes, keys == vals == the image.  Asynchronous on ``stream``."""
        _lib.check(self.lib.lsmck_wal_recs_to_cmds(self.handle, recs_ptr, n, img_bytes, cmds_ptr, stream),
                   "wal_recs_to_cmds")

    def wal_replay_verify(self, image, device_ptr=None, cap=None, pinned_recs=False, compact=False):
        """Returns (records, status, (bad_index, bad_crc, bad_expected)).
        cap: records to return at most (default: the n/9 + 1 a log of n
        bytes can hold; a very large log whose record count is known can ask
        for fewer -- the status and the count cover the whole log).
        pinned_recs: the records land in a page-locked array by DMA
        (LSMCK_RECS_PINNED; cap entries stay pinned for the context's life).
        compact: 16-byte records (lsmck_wal_replay_verify16, WAL_REC16_DTYPE;
        decode_rec16 gives the 32-byte form's fields)."""
        if device_ptr is None:
            # any buffer (bytes, bytearray, memoryview, a read-only mmap of the
            # log file) is read in place: no copy of the image
            img = np.frombuffer(image, dtype=np.uint8) if len(image) else np.zeros(1, dtype=np.uint8)[:0]
            ptr, n, flags = img.ctypes.data, len(img), _lib.HOST
        else:
            ptr, n, flags = device_ptr, image, _lib.DEVICE
        cap = n // 9 + 1 if cap is None else cap  # a record is at least 9 bytes (Remove of an empty key)
        dtype = WAL_REC16_DTYPE if compact else WAL_REC_DTYPE
        if pinned_recs:
            recs = self._wal_recs_pinned(cap, dtype)
            flags |= _lib.RECS_PINNED
        else:
            recs = self._wal_recs_buffer(cap, dtype)
        nrec = C.c_size_t()
        bi, bc, be = C.c_uint64(), C.c_uint32(), C.c_uint32()
        fn = self.lib.lsmck_wal_replay_verify16 if compact else self.lib.lsmck_wal_replay_verify
        rc = _lib.check(fn(self.handle, ptr, n, flags, recs.ctypes.data, cap, C.byref(nrec), C.byref(bi),
                           C.byref(bc), C.byref(be)), "wal_replay_verify")
        # np.recarray: record fields read as attributes (r.payload_off), like the ctypes struct
        # nrec counts the whole log's accepted records; at most cap of them were written
        return recs[:min(nrec.value, cap)].view(np.recarray), rc, (bi.value, bc.value, be.value)

    def wal_replay_verify_to_device(self, image, recs_ptr, cap, device_ptr=None, compact=False):
        """The replay with its records left in device memory (LSMCK_RECS_DEVICE):
        recs_ptr is a device array of cap lsmck_wal_rec entries (32 bytes each,
        WAL_REC_DTYPE; compact: lsmck_wal_rec16, 16 bytes, WAL_REC16_DTYPE).
        Returns (nrec, status, (bad_index, bad_crc, bad_expected)); min(nrec, cap)
        records were written."""
        if device_ptr is None:
            img = np.frombuffer(image, dtype=np.uint8) if len(image) else np.zeros(1, dtype=np.uint8)[:0]
            ptr, n, flags = img.ctypes.data, len(img), _lib.HOST
        else:
            ptr, n, flags = device_ptr, image, _lib.DEVICE
        nrec = C.c_size_t()
        bi, bc, be = C.c_uint64(), C.c_uint32(), C.c_uint32()
        fn = self.lib.lsmck_wal_replay_verify16 if compact else self.lib.lsmck_wal_replay_verify
        rc = _lib.check(fn(self.handle, ptr, n, flags | _lib.RECS_DEVICE, recs_ptr, cap, C.byref(nrec), C.byref(bi),
                           C.byref(bc), C.byref(be)), "wal_replay_verify")
        return nrec.value, rc, (bi.value, bc.value, be.value)

    def checksums_verify_many(self, triples):
        n = len(triples)
        arr = C.c_char_p * max(n, 1)
        d = arr(*[str(t[0]).encode() for t in triples])
        i = arr(*[str(t[1]).encode() for t in triples])
        c = arr(*[str(t[2]).encode() for t in triples])
        status = (C.c_int * max(n, 1))()
        _lib.check(self.lib.lsmck_checksums_verify_many(self.handle, d, i, c, n, status), "checksums_verify_many")
        return list(status[:n])

    def tree_verify(self, base, listed=None):
        """lsmck_tree_verify: Db::load's table scan + batch verify of the tree
        under ``base``.  Returns a dict of the report (first_* describe the
        first failing table in load order, or are None).  ``listed``: a list
        that receives the verify's listing (lsmck_tree_verify_listed), one
        dict per table in load order, before the tables are hashed."""
        rep = _lib.TreeReport()
        if listed is None:
            rc = self.lib.lsmck_tree_verify(self.handle, str(base).encode(), C.byref(rep))
        else:
            def on_listed(_user, e, n):
                for i in range(n):
                    t = e[i]
                    dec = lambda b: b.decode(errors="surrogateescape") if b is not None else None  # noqa: E731
                    listed.append({"metadata_path": dec(t.metadata_path), "data_path": dec(t.data_path),
                                   "index_path": dec(t.index_path), "checksum_path": dec(t.checksum_path),
                                   "id": dec(t.id), "level": t.level, "status": t.status})
            fn = _lib.LISTED_FN(on_listed)
            rc = self.lib.lsmck_tree_verify_listed(self.handle, str(base).encode(), C.byref(rep), fn, None)
        return _tree_report(rep, _lib.check(rc, "tree_verify"))


def _tree_report(rep, rc):
    """lsmck_tree_report as a dict (first_* are None when every table verified)."""
    bad = rc != 0
    return {"tables": rep.tables, "table_bytes": rep.table_bytes, "bad_tables": rep.bad_tables,
            "first_index": rep.first_index if bad else None, "first_status": rep.first_status if bad else None,
            "first_metadata_path": rep.first_metadata_path.decode(errors="surrogateescape") if bad else None,
            "list_seconds": rep.list_seconds, "verify_seconds": rep.verify_seconds,
            "stat_seconds": rep.stat_seconds, "read_seconds": rep.read_seconds,
            "gpu_wait_seconds": rep.gpu_wait_seconds, "compare_seconds": rep.compare_seconds,
            "rounds": rep.rounds, "fds_cached": rep.fds_cached}


def _path_arrays(triples):
    n = len(triples)
    arr = C.c_char_p * max(n, 1)
    return (arr(*[str(t[0]).encode() for t in triples]), arr(*[str(t[1]).encode() for t in triples]),
            arr(*[str(t[2]).encode() for t in triples]))


class MultiContext:
    """Host-resident batches split over several GPUs in one process (SURVEY
    8e): one Context per device, one host thread each (the ctypes calls drop
    the GIL), contiguous record ranges -- by bytes for variable-length records
    (shard.shard_by_bytes), by count for fixed ones -- and no data exchange
    between devices: each device's results land in its slice of the output.
    Each device's host path streams its share through its own pinned slots,
    so the PCIe links of the devices work in parallel."""

    def __init__(self, devices=None, contexts=None):
        if contexts is None:
            devices = range(device_count()) if devices is None else devices
            contexts = [Context(d) for d in devices]
        if not contexts:
            raise _lib.LsmckError(_lib.ENODEV, "MultiContext: no device")
        self.ctxs = list(contexts)

    def _parallel(self, bounds, fn):
        import concurrent.futures as cf
        with cf.ThreadPoolExecutor(len(self.ctxs)) as ex:
            for f in [ex.submit(fn, k, int(bounds[k]), int(bounds[k + 1])) for k in range(len(self.ctxs))]:
                f.result()

    def _var(self, data, off, length, width, call):
        off = np.ascontiguousarray(off, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint32)
        out = np.empty((len(off), width) if width > 1 else len(off), dtype=np.uint8 if width > 1 else np.uint32)
        b = shard_by_bytes(length, len(self.ctxs))

        def part(k, r0, r1):
            if r1 > r0:
                out[r0:r1] = call(self.ctxs[k], data, off[r0:r1], length[r0:r1])
        self._parallel(b, part)
        return out

    def _fixed(self, data, stride, length, n, width, call):
        out = np.empty((n, width) if width > 1 else n, dtype=np.uint8 if width > 1 else np.uint32)
        b = [shard_fixed(n, len(self.ctxs), k)[0] for k in range(len(self.ctxs))] + [n]
        data = np.ascontiguousarray(data, dtype=np.uint8)

        def part(k, r0, r1):
            if r1 > r0:
                out[r0:r1] = call(self.ctxs[k], data[r0 * stride:], stride, length, r1 - r0)
        self._parallel(b, part)
        return out

    def crc32(self, data, off, length):
        return self._var(np.ascontiguousarray(data, dtype=np.uint8), off, length, 1, Context.crc32)

    def crc32_fixed(self, data, stride, length, n):
        return self._fixed(data, stride, length, n, 1, Context.crc32_fixed)

    def sha256(self, data, off, length):
        return self._var(np.ascontiguousarray(data, dtype=np.uint8), off, length, 32, Context.sha256)

    def sha256_fixed(self, data, stride, length, n):
        return self._fixed(data, stride, length, n, 32, Context.sha256_fixed)

    # --- SSTable verify over every device's PCIe link (lsmck_*_multi) ---------
    def _handles(self):
        return (C.c_void_p * len(self.ctxs))(*[c.handle for c in self.ctxs])

    def checksums_verify_many(self, triples):
        n = len(triples)
        d, i, c = _path_arrays(triples)
        status = (C.c_int * max(n, 1))()
        lib = _lib.load()
        _lib.check(lib.lsmck_checksums_verify_many_multi(self._handles(), len(self.ctxs), d, i, c, n, status),
                   "checksums_verify_many_multi")
        return list(status[:n])

    def tree_verify(self, base):
        rep = _lib.TreeReport()
        lib = _lib.load()
        rc = _lib.check(lib.lsmck_tree_verify_multi(self._handles(), len(self.ctxs), str(base).encode(),
                                                    C.byref(rep)), "tree_verify_multi")
        return _tree_report(rep, rc)

    def wal_replay_verify(self, image, device_ptr=None, cap=None, pinned_recs=False, compact=False):
        """The WAL is one log: replayed on the first device (Context.wal_replay_verify)."""
        return self.ctxs[0].wal_replay_verify(image, device_ptr, cap=cap, pinned_recs=pinned_recs, compact=compact)


# include/lsmck.h lsmck_wal_rec (32 bytes, no padding)
WAL_REC_DTYPE = np.dtype([("rec_off", "<u8"), ("payload_off", "<u8"), ("klen", "<u4"), ("vlen", "<u4"),
                          ("crc", "<u4"), ("type", "<u4")])
assert WAL_REC_DTYPE.itemsize == C.sizeof(_lib.WalRec)
# include/lsmck.h lsmck_wal_rec16 (16 bytes): lsmck_wal_replay_verify16's compact records
WAL_REC16_DTYPE = np.dtype([("payload_type", "<u8"), ("klen", "<u4"), ("vlen", "<u4")])
assert WAL_REC16_DTYPE.itemsize == C.sizeof(_lib.WalRec16)


def decode_rec16(recs):
    """Compact records as the 32-byte form's fields: a dict of arrays rec_off,
    payload_off, klen, vlen, type (the stored CRC is not kept: it is the
    computed one for every accepted record)."""
    pt = np.asarray(recs["payload_type"], dtype=np.uint64)
    remove = (pt >> np.uint64(63)).astype(bool)
    payload = pt & np.uint64(_lib.WAL_REC16_REMOVE - 1)
    typ = np.where(remove, 2, 1).astype(np.uint32)
    return {"rec_off": payload - np.where(remove, 9, 13).astype(np.uint64), "payload_off": payload,
            "klen": np.asarray(recs["klen"]), "vlen": np.asarray(recs["vlen"]), "type": typ}


def device_count():
    return _lib.load().lsmck_device_count()


def gen_zipf_lengths(seed, n, s=1.5, kmax=1024, lmin=64, first=0):
    """lengths of records [first, first + n) of the config-3 length stream"""
    out = np.empty(n, dtype=np.uint32)
    _lib.load().lsmck_gen_zipf_lengths_at(seed, s, kmax, lmin, first, n, out.ctypes.data)
    return out
