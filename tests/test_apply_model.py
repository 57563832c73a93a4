"""The batch command stream's shared logic (csrc/lsmck_apply.h: the validation
with Gets, the packed words, the two max-scans' words and prev / ans / pq from
their outputs, the forward entry flags, the slots and the answers -- the code
the kernels of lsmck_apply.hip run) as a host model under AddressSanitizer and
UBSan (host code only; g++, a stand-alone program): tests/native/test_apply.cpp
runs every step in the kernels' order around the write plan's own steps, with
caps, block sizes and window widths from 1 up, streams of only Gets, of one
key and of memtables longer than two windows, and compares with the literal
loop over std::maps, the arenas exact-size blocks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_apply_model_asan(tmp_path):
    exe = tmp_path / "apply"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_apply.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "apply ok" in r.stdout
