"""The batch WAL encode's gather logic (csrc/lsmck_walenc.h: the code the
kernel wal_encode_gather runs per tile and per chunk) as a host model under
AddressSanitizer and UBSan (host code only; g++): tests/native/test_walenc.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walenc_model_asan(tmp_path):
    exe = tmp_path / "walenc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_walenc.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "walenc ok" in r.stdout
