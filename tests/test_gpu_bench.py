"""bench.py's N-rank path and BASELINE config 4 on the GPU.

* `python bench.py --gpus 2` (no launcher) must start two ranks itself
  (torch.distributed.run as a child process), report n_gpus 2 and the config-3
  workload -- rank r = records [r*n, (r+1)*n) of one global stream -- and
  every rank's shard must match the oracle's digest (committed:
  tests/golden/summaries.json config3_shards_small); its config-4 sub-line
  likewise (digests computed here).  The two ranks share the box's one GPU
  (LSMCK_BENCH_SHARE_GPU=1) on reduced shards.  --config 2 keeps the
  config-4 shard as the main line.  These lines are read from `--full` runs:
  the digests and the config-4 sub-line are not part of a plain run.
* A plain run (`--gpus 1 --steps K --warmup W`) carries the headline fields
  only, and `--dump-outputs DIR` holds the last timed step's CRCs.
* Config 4's per-GPU shard at full size (2^26 x 4 KiB = 256 GiB, rank 0's
  blocks [0, 2^26) of config 2's stream) through the C ABI, against the
  oracle's summary digest (tests/golden/make_summaries.py config4).
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED2 = 0x5EED0002


def _oracle_shard_summary(rank, nrec, threads=16):
    data = O.gen_stream(SEED2, rank * nrec * 4096, nrec * 4096)
    crc = O.crc32_fixed(data, 4096, 4096, nrec, threads=threads)
    return "%08x" % zlib.crc32(crc.astype("<u4").tobytes())


def _bench2(*args, gpus=2, timeout=300):
    env = dict(os.environ, LSMCK_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "3",
                        "--warmup", "1", "--full", *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_gpus2_config3_global_stream():
    """The default N-rank line: config 3 on both ranks, each its own segment of
    one global stream (2^20 records per rank here), digests equal to the
    oracle's; the config-4 sub-line's shards too."""
    nrec, n4 = 1 << 20, 1 << 18
    r = _bench2("--blocks-per-gpu", str(nrec), "--c4-blocks", str(n4))
    assert r["n_gpus"] == 2 and r["scaling"] == "weak"
    assert r["config"]["workload"].startswith("config3")
    assert r["config"]["records_per_gpu"] == nrec
    with open(os.path.join(ROOT, "tests", "golden", "summaries.json")) as f:
        g = json.load(f)["config3_shards_small"]
    assert r["rank_summaries_crc32"] == g["shard_summary_crc32"][:2]
    assert r["summary_matches_oracle"] is True
    # value = both ranks' payload over the slowest rank's time
    pay = sum(g["shard_bytes"][:2])
    assert abs(r["value"] - pay / 2**30 / (r["ms_per_step"] * 1e-3)) / r["value"] < 0.01
    c4 = r["config4"]
    assert c4["records_per_gpu"] == n4
    assert [p["summary_crc32"] for p in c4["per_rank"]] == [_oracle_shard_summary(k, n4) for k in range(2)]
    assert abs(c4["value"] - 2 * n4 * 4096 / 2**30 / (c4["ms_per_step"] * 1e-3)) / c4["value"] < 0.01


@pytest.mark.gpu
def test_bench_gpus8_rehearsal():
    """The 8-rank line before the driver's 8-GPU node runs it: eight ranks on
    the box's one GPU (LSMCK_BENCH_SHARE_GPU=1), reduced shards.  Every
    rank's config-3 shard -- records [r*2^20, (r+1)*2^20) of one global
    stream -- equals the committed oracle digest, every rank's config-4 shard
    the oracle's (computed here), and value is all ranks' payload over the
    slowest rank's time."""
    nrec, n4 = 1 << 20, 1 << 18
    r = _bench2("--blocks-per-gpu", str(nrec), "--c4-blocks", str(n4), gpus=8, timeout=600)
    assert r["n_gpus"] == 8 and r["scaling"] == "weak"
    assert r["config"]["workload"].startswith("config3")
    with open(os.path.join(ROOT, "tests", "golden", "summaries.json")) as f:
        g = json.load(f)["config3_shards_small"]
    assert len(g["shard_summary_crc32"]) == 8
    assert r["rank_summaries_crc32"] == g["shard_summary_crc32"]
    assert r["summary_matches_oracle"] is True
    pay = sum(g["shard_bytes"][:8])
    assert abs(r["value"] - pay / 2**30 / (r["ms_per_step"] * 1e-3)) / r["value"] < 0.01
    c4 = r["config4"]
    assert [p["summary_crc32"] for p in c4["per_rank"]] == [_oracle_shard_summary(k, n4) for k in range(8)]
    assert abs(c4["value"] - 8 * n4 * 4096 / 2**30 / (c4["ms_per_step"] * 1e-3)) / c4["value"] < 0.01


@pytest.mark.gpu
def test_bench_gpus2_launches_two_ranks():
    nrec = 1 << 18  # 1 GiB per rank
    env = dict(os.environ, LSMCK_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "2",
                        "--blocks-per-gpu", str(nrec), "--steps", "3", "--warmup", "1", "--full"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    r = json.loads(line)
    assert r["n_gpus"] == 2
    assert r["config"]["workload"].startswith("config4")
    assert r["config"]["records_per_gpu"] == nrec
    assert r["scaling"] == "weak"
    want = [_oracle_shard_summary(k, nrec) for k in range(2)]
    assert r["rank_summaries_crc32"] == want
    # the N > 1 line is evaluable: PMC traffic (config 4's, scaled to the
    # reduced shard) and every rank's own launch time
    assert r["roofline"]["traffic"] is not None and r["roofline"]["traffic"] > 0
    assert [p["rank"] for p in r["per_rank"]] == [0, 1]
    lo, hi = r["roofline"]["launch_ms_min_max_over_ranks"]
    assert 0 < lo <= hi
    assert all(0 < p["frac"] < 1 for p in r["per_rank"])
    assert [p["summary_crc32"] for p in r["per_rank"]] == want
    # value = both ranks' payload over the slowest rank's time
    assert abs(r["value"] - 2 * nrec * 4096 / 2**30 / (r["ms_per_step"] * 1e-3)) / r["value"] < 0.01


def test_bench_default_workload_is_config3():
    """Every N defaults to BASELINE config 3 (north_star's 64 B-64 KiB records
    at 1, 2, 4 and 8 GPUs): the 1 -> N curve is like for like."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.resolve_config(0, 1) == 3
    assert bench.resolve_config(0, 8) == 3
    assert bench.resolve_config(2, 8) == 2


def test_bench_world_size_mismatch_fails():
    """Under a launcher, WORLD_SIZE must equal --gpus (checked before any GPU call)."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2
    assert "WORLD_SIZE=2" in p.stderr


class _HostOut:
    """dump_outputs' view of a device buffer, over host bytes"""

    def __init__(self, raw):
        self.raw = np.ascontiguousarray(raw).view(np.uint8)

    def download(self, dtype=np.uint8, count=None, offset=0):
        return self.raw.view(dtype)[:count].copy()


def test_bench_dump_outputs_whole(tmp_path):
    """--dump-outputs: an output inside the budget is dumped whole, as float64."""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(7)
    crc = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    bench.dump_outputs(str(tmp_path / "a"), _HostOut(crc), crc.size, False, 0)
    got = np.load(tmp_path / "a" / "crc32.npy")
    assert got.dtype == np.float64 and np.array_equal(got, crc.astype(np.float64))
    dig = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), _HostOut(dig), 50, True, 3)
    got = np.load(tmp_path / "a" / "sha256_rank3.npy")
    assert got.dtype == np.float64 and np.array_equal(got, dig.astype(np.float64))


MULT = 2654435761  # odd: i -> i * MULT mod 2^32 is one to one, so a dumped value names its record


def _records_of(values):
    return (values.astype(np.uint64) * np.uint64(pow(MULT, -1, 1 << 32))) % np.uint64(1 << 32)


def test_bench_dump_outputs_sample(tmp_path):
    """A large output is dumped as a sample: the same one every time, float64,
    distinct records in index order, one from every stratum of the batch (so it
    spans the whole output), and all ranks' files together under 64 MB."""
    sys.path.insert(0, ROOT)
    import bench
    keep = bench.DUMP_MAX_BYTES // 8
    n = 3 * keep + 7
    big = (np.arange(n, dtype=np.uint64) * np.uint64(MULT) % np.uint64(1 << 32)).astype(np.uint32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), _HostOut(big), n, False, 0)
    b, c = np.load(tmp_path / "b" / "crc32.npy"), np.load(tmp_path / "c" / "crc32.npy")
    assert b.dtype == np.float64 and b.shape == (keep,) and np.array_equal(b, c)
    assert os.path.getsize(tmp_path / "b" / "crc32.npy") <= 64 * 10**6
    idx = _records_of(b)
    assert np.all(np.diff(idx.astype(np.int64)) > 0) and idx[-1] < n
    edges = (np.arange(keep + 1, dtype=np.uint64) * np.uint64(n)) // np.uint64(keep)
    assert np.all(idx >= edges[:-1]) and np.all(idx < edges[1:])
    assert np.any(idx != edges[:-1])  # drawn, not a plain stride
    # one past the limit still samples, and exactly `keep` distinct records
    bench.dump_outputs(str(tmp_path / "d"), _HostOut(big), keep + 1, False, 0)
    d = _records_of(np.load(tmp_path / "d" / "crc32.npy"))
    assert d.shape == (keep,) and np.all(np.diff(d.astype(np.int64)) > 0) and d[-1] <= keep
    # N ranks share the budget: every rank's file counted
    for world in (2, 8):
        out = tmp_path / f"w{world}"
        for rank in range(world):
            bench.dump_outputs(str(out), _HostOut(big), n, False, rank, world)
        files = sorted(os.listdir(out))
        assert files == sorted(["crc32.npy"] + [f"crc32_rank{r}.npy" for r in range(1, world)])
        assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10**6
        for f in files:
            r = _records_of(np.load(out / f))
            assert r.shape == (keep // world,) and np.all(np.diff(r.astype(np.int64)) > 0) and r[-1] < n
    dig = np.repeat(big[:keep // 8].view(np.uint8).reshape(-1, 4), 8, axis=1)  # [n, 32] digests
    bench.dump_outputs(str(tmp_path / "s"), _HostOut(dig), dig.shape[0], True, 0)
    s = np.load(tmp_path / "s" / "sha256.npy")
    assert s.dtype == np.float64 and s.shape == (keep // 32, 32) and s.nbytes <= bench.DUMP_MAX_BYTES
    sidx = _records_of(np.ascontiguousarray(s[:, ::8].astype(np.uint8)).view(np.uint32).ravel())
    assert np.all(np.diff(sidx.astype(np.int64)) > 0) and sidx[-1] < dig.shape[0]
    assert np.array_equal(s, dig[sidx.astype(np.int64)].astype(np.float64))


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run carries the headline fields and none of --full's legs, takes
    --steps timed steps, and --dump-outputs holds the last step's CRCs: every
    record's equals the oracle's."""
    nrec = 1 << 14
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--blocks-per-gpu", str(nrec), "--dump-outputs", str(tmp_path)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert r["steps"] == 4 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["unit"] == "GiB/s" and r["higher_is_better"] is True and r["dtype"] == "u8"
    assert r["metric"].startswith("GiB/s device-resident batched record checksum")
    assert r["config"]["workload"].startswith("config3") and r["config"]["records_per_gpu"] == nrec
    assert r["ms_per_step"] > 0
    pay = r["config"]["payload_bytes_per_gpu"]
    assert abs(r["value"] - pay / 2**30 / (r["ms_per_step"] * 1e-3)) / r["value"] < 0.01
    assert r["cpu_baseline"] is None
    for k in ("config4", "host_roundtrip", "cpu_extra", "summary_crc32", "summary_matches_oracle"):
        assert k not in r
    assert "loads_only_ceiling" not in r["roofline"]
    lens = O.gen_zipf_lengths(0x5EED0003, nrec)
    offs = np.zeros(nrec, dtype=np.uint64)
    np.cumsum(lens[:-1].astype(np.uint64), out=offs[1:])
    data = O.gen_stream(0x5EED0003, 0, int(offs[-1]) + int(lens[-1]))
    got = np.load(tmp_path / "crc32.npy")
    assert got.dtype == np.float64
    assert np.array_equal(got, O.crc32_batch(data, offs, lens).astype(np.float64))


@pytest.mark.gpu
def test_bench_dump_outputs_sampled_on_gpu(tmp_path):
    """An output past the dump budget (config 1, 2^22 + 8 records of 256 B: 8
    records over) is dumped as 2^22 sampled CRCs: sample i is the oracle's CRC
    of a record in stratum i of the batch."""
    sys.path.insert(0, ROOT)
    import bench
    keep = bench.DUMP_MAX_BYTES // 8
    nrec = keep + 8
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "1", "--blocks-per-gpu", str(nrec), "--dump-outputs", str(tmp_path)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert r["config"]["records_per_gpu"] == nrec and r["steps"] == 2
    got = np.load(tmp_path / "crc32.npy")
    assert got.dtype == np.float64 and got.shape == (keep,)
    want = O.crc32_fixed(O.gen_stream(0x5EED0001, 0, nrec * 256), 256, 256, nrec, threads=16).astype(np.float64)
    edges = (np.arange(keep + 1, dtype=np.uint64) * np.uint64(nrec)) // np.uint64(keep)
    lo, hi = edges[:-1].astype(np.int64), edges[1:].astype(np.int64)
    assert (hi - lo).max() <= 2  # so a stratum is its first and last record
    assert np.all((got == want[lo]) | (got == want[hi - 1]))


@pytest.mark.gpu
def test_config4_rank0_shard_full_size(ctx):
    """2^26 x 4 KiB = 256 GiB on one GPU, every CRC checked through the summary digest."""
    with open(os.path.join(ROOT, "tests", "golden", "summaries.json")) as f:
        want = json.load(f)["config4"]["shard_summary_crc32"][0]
    n = 1 << 26
    d = ctx.alloc(n * 4096)
    out = ctx.alloc(4 * n)
    try:
        ctx.gen_stream(d.ptr, SEED2, 0, n * 4096)
        ctx.crc32_fixed_device(d.ptr, 4096, 4096, n, out.ptr)
        ctx.sync()
        crc = out.download(np.uint32)
        assert "%08x" % zlib.crc32(crc.astype("<u4").tobytes()) == want
        # and a spread sample against the oracle record by record
        idx = np.linspace(0, n - 1, 512).astype(np.int64)
        for i in idx[::64]:
            blk = O.gen_stream(SEED2, int(i) * 4096, 4096)
            assert crc[i] == O.crc32(blk)
    finally:
        d.free()
        out.free()
