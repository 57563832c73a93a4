"""The batch Db::get's shared logic (csrc/lsmck_dbget.h: the run pass, the run
probe's two-arena lower bound, resolve with the answered lengths, and the
gather's tile search, slice and chunks -- the code the kernels of
lsmck_dbget.hip run -- with csrc/lsmck_sstget.h for the tables) as a host model
under AddressSanitizer and UBSan (host code only; g++, a stand-alone program,
no Python under a sanitizer): tests/native/test_dbget.cpp runs the kernels'
steps in order, the pairs in both orders and the gather lane by lane, and
compares with a std::map per source and a loop over bytes, the arenas
exact-size blocks with keys and values flush against both ends."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dbget_model_asan(tmp_path):
    exe = tmp_path / "dbget"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_dbget.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "dbget ok" in r.stdout
