"""The stream kernel's slice plan (csrc/lsmck_splan.h) for the tests: builds
tests/native/splan_export.cpp with g++ into a temporary shared object once per
process and binds it.  No GPU and no liblsmck.so needed."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def load():
    gxx = shutil.which("g++")
    if gxx is None:
        raise RuntimeError("the slice-plan model needs g++ to build tests/native/splan_export.cpp")
    d = tempfile.mkdtemp(prefix="splan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "splan.so")
    subprocess.run([gxx, "-O1", "-std=c++17", "-shared", "-fPIC",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "splan_export.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.splan_fraction.restype = C.c_double
    lib.splan_fraction.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    lib.splan_slices.restype = C.c_uint32
    lib.splan_slices.argtypes = [C.c_int, C.c_uint64]
    lib.splan_slices_max.restype = C.c_uint32
    lib.splan_slices_max.argtypes = [C.c_int]
    lib.splan_waves.restype = C.c_uint32
    lib.splan_waves.argtypes = [C.c_int]
    return lib


def cuts(ncu, off, lens, targets=False):
    """The records at which stream_cut cuts a batch (numpy off / lens): cut w is
    the first record starting at or after off[0] + span * fraction(w) (with
    `targets`, those byte targets too)."""
    import numpy as np
    lib = load()
    n = len(off)
    S, W = lib.splan_slices(ncu, n), lib.splan_waves(ncu)
    o0, dend = int(off[0]), int(off[-1]) + int(lens[-1])
    span = float(dend - o0)
    target = np.array([o0 + int(span * lib.splan_fraction(w, S, W)) for w in range(S)], dtype=np.uint64)
    cut = np.append(np.searchsorted(off, target, side="left"), n)
    return (cut, target) if targets else cut


def first_n_over_one_slice_per_wave(ncu):
    """The smallest record count at which a batch gets more slices than waves."""
    lib = load()
    w = lib.splan_waves(ncu)
    lo, hi = 1, 1 << 40  # slices(lo) == w < slices(hi); slices() is monotone in n
    assert lib.splan_slices(ncu, lo) == w < lib.splan_slices(ncu, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.splan_slices(ncu, mid) > w:
            hi = mid
        else:
            lo = mid
    return hi
