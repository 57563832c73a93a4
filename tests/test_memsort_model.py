"""The batch memtable build's shared logic (csrc/lsmck_memsort.h: the validity
rule, chunk_tail with its dword-load rule, the regroup predicate, the
mem_bytes shares and the adapter's record conversion -- the code the kernels
of lsmck_memtable.hip run) as a host model under AddressSanitizer and UBSan
(host code only; g++, a stand-alone program): tests/native/test_memsort.cpp
runs the whole refinement with std::stable_sort in place of the device's radix
sort and compares with a std::map, the key arena an exact-size block with keys
flush against both ends."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memsort_model_asan(tmp_path):
    exe = tmp_path / "memsort"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_memsort.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "memsort ok" in r.stdout
