"""The opened table set's bloom filters (csrc/lsmck_bloom.h: the hash, the
split-block arithmetic, the count and fill walks, the interval <-> table
mapping and the filtered probe -- the code the kernels of lsmck_tableset.hip
run) as a host model under AddressSanitizer and UBSan (host code only; g++, a
stand-alone program, no Python under a sanitizer): tests/native/test_bloom.cpp
opens random and doctored tables at the caps 1, 4 and 256 and 4, 12 and 64
bits per key, runs the probe in kernel order with the pairs in both orders,
and compares with the same get without filters, with get::table_get and with
a std::map, the arenas and the filter buffers exact-size blocks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bloom_model_asan(tmp_path):
    exe = tmp_path / "bloom"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_bloom.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "bloom ok" in r.stdout
