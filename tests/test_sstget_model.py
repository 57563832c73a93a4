"""The batch point read's shared logic (csrc/lsmck_sstget.h: the map's parse,
the order keys and the order check, the lower bound with its tie path, the
exact hit, the interval scan, the winner's minimum and resolve -- the code the
kernels of lsmck_sstget.hip run) as a host model under AddressSanitizer and
UBSan (host code only; g++, a stand-alone program, no Python under a
sanitizer): tests/native/test_sstget.cpp runs the kernels' steps in order and
compares with a std::map and loops over bytes, the arenas exact-size blocks
with tables and query keys flush against both ends."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sstget_model_asan(tmp_path):
    exe = tmp_path / "sstget"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_sstget.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "sstget ok" in r.stdout
