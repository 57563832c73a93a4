"""The batch write plan's shared logic (csrc/lsmck_writeplan.h: the size rule,
prev and the packed words, the capped walk, the in-block links, the window's
delta and flush test, the entry predicate and the entry itself -- the code the
kernels of lsmck_writeplan.hip run) as a host model under AddressSanitizer and
UBSan (host code only; g++, a stand-alone program):
tests/native/test_writeplan.cpp runs every step in the kernels' order, with
caps, block sizes and window widths from 1 up -- and 2500 and 3100 commands
with windows of 1000 and 1024 in blocks of 1024, 1025 and 8192, memtables of
more than two windows --, and compares with the literal loop over a std::map,
the arenas exact-size blocks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_writeplan_model_asan(tmp_path):
    exe = tmp_path / "writeplan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_writeplan.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "writeplan ok" in r.stdout
