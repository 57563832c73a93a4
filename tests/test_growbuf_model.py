"""The host layer's owning, grow-only buffer (csrc/lsmck_buf.h: every device and
pinned scratch buffer of a context is one) under AddressSanitizer and UBSan
(host code only; g++, a stand-alone program): tests/native/test_growbuf.cpp
instantiates it over a counting malloc that can fail on demand and checks the
growth rule (need, or 3/2 of the capacity; at least one element), that a plain
growth frees before it allocates, what a failed growth leaves, ensure_keep,
moves, and that every block is freed exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_growbuf_model_asan(tmp_path):
    exe = tmp_path / "growbuf"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_growbuf.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "growbuf ok" in r.stdout
