"""The batch SSTable decode and merge's shared logic (csrc/lsmck_sstmerge.h: the
record step, the index parse, the hint's acceptance rule, the lower bound with
its order-key fast path, the winner and tombstone rules -- the code the kernels
of lsmck_sstmerge.hip run) as a host model under AddressSanitizer and UBSan
(host code only; g++, a stand-alone program, no Python under a sanitizer):
tests/native/test_sstmerge.cpp runs the kernels' steps in order and compares
with a byte-by-byte iterator and a std::map, the arenas exact-size blocks with
tables flush against both ends."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sstmerge_model_asan(tmp_path):
    exe = tmp_path / "sstmerge"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_sstmerge.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "sstmerge ok" in r.stdout
