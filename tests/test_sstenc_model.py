"""The batch SSTable encode's gather logic (csrc/lsmck_sstenc.h: the code the
kernel sst_gather runs per tile and per chunk, the record arithmetic and the
key order) as a host model under AddressSanitizer and UBSan (host code only;
g++, a stand-alone program): tests/native/test_sstenc.cpp, with the kernel's
tile and with tiles of 256 bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tile", [None, 256])
def test_sstenc_model_asan(tmp_path, tile):
    exe = tmp_path / "sstenc"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                   ([f"-DLSMCK_SST_TILE={tile}u"] if tile else []) +
                   ["-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_sstenc.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert f"sstenc ok (tile {tile or 32768})" in r.stdout
