"""A destroyed context gives its device memory back: tools/ctx_cycle.py creates
a context, takes every path that grows one of its buffers (host and device
batches, every WAL walk, the three batch builders in host form, a table
verify; each result checked against the oracle or the CPU path) and closes
it, three times over, reading the device's free memory after each cycle.  The
tool runs as a fresh child process: it imports torch before the library.

Free memory after cycle 3 may be below free memory after cycle 2 by what it
was on the commit that still freed every buffer by hand (0 bytes, measured
with this tool: profiles/r10/refactor/README.md) plus 2 MiB.  The cycle's
larger buffers are each above 2 MiB, so one of them leaking fails here;
smaller buffers are tests/test_growbuf_model.py's and the reviewer's."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_DROP = 0  # bytes, the parent commit's drop between cycles 2 and 3
MARGIN = 2 << 20


@pytest.mark.gpu
def test_context_cycles_return_device_memory():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ctx_cycle.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    print(r)
    assert r["cycles"] == 3 and r["results_checked"] and len(r["free_bytes_after_cycle"]) == 3
    free = r["free_bytes_after_cycle"]
    assert free[1] - free[2] <= PARENT_DROP + MARGIN, r
