"""lsmck_ctx_set_option's options as data (csrc/lsmck_options.h: the values with
their defaults, one table row per option, one function that looks a key up,
checks the value and stores it) under AddressSanitizer and UBSan (host code
only; g++, a stand-alone program): tests/native/test_options.cpp holds its own
hand-written table of every option's default and accepted values and checks
both ends of each range, the refusals (LSMCK_EINVAL, nothing stored), the
`variant` bits of crc_stream / sha_order / crc_ablate, and the two ranges that
depend on the device (wal_pipe_cus) and on the build (crc_ablate)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_model_asan(tmp_path):
    exe = tmp_path / "options"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "lsm_storage_engine_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "test_options.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "options ok" in r.stdout
