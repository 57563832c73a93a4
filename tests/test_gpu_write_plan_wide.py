"""lsmck_db_write_plan on the GPU where test_gpu_write_plan.py's small settings
do not reach: LONG memtables of more than one of the chain's windows of 1024
commands (write_cases.windows: the carry from window to window, the partial
last window, negative deltas in the scan, the first qualifying Insert across
sixteen waves), and streams of more than two default blocks at cut_block 8192
down to 65 (write_cases.wide: wpl_exit with up to eight links a thread and
thirteen doubling rounds, block widths that are no power of two, wpl_mark with
more entry points in a block than threads).  The expected values are the cases
module's (wal.MemTable.insert command by command; tests/test_write_cases.py
proves on the CPU that the streams reach these edges), the comparison is
test_gpu_write_plan.check_stream's: exact, outputs between intact 0xAA guards,
cut_long the restatement's LONG count, cut_steps <= n * cut_walk_cap."""
import pytest

import write_cases as Wc
from test_gpu_write_plan import check_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(ctx):
    yield
    ctx.set_option("cut_block", Wc.DEFAULT_BLOCK)
    ctx.set_option("cut_walk_cap", Wc.DEFAULT_CAP)


def at_block(s, block):
    t = s.at(name=f"{s.name}@block{block}")
    t.block = block
    return t


# --- the chain's windows ---------------------------------------------------------------------------
@pytest.mark.parametrize("s", Wc.windows(), ids=lambda s: s.name)
def test_window_stream(ctx, s):
    """With blocks of 64 and with the whole stream in one default block."""
    assert s.block == Wc.BLOCK and len(s) > Wc.W and s.expected().long_count(s.cap) >= 1
    a = check_stream(ctx, s)
    b = check_stream(ctx, at_block(s, Wc.DEFAULT_BLOCK))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_big_closes_memtables_longer_than_a_window(ctx):
    """2^18 commands over 2^12 keys at a limit of 32 KiB: 89 closed memtables of two and three windows."""
    s = Wc.big(Wc.BIG_WINDOW_LIMIT)
    assert sum(1 for ln in s.expected().lens[:-1] if ln > Wc.W) >= 10
    check_stream(ctx, s)


# --- the block widths --------------------------------------------------------------------------------
@pytest.mark.parametrize("s", Wc.wide(), ids=lambda s: s.name)
def test_wide_stream_at_every_block_width(ctx, s):
    assert s.block == Wc.DEFAULT_BLOCK
    first = None
    for block in Wc.WIDE_BLOCKS:
        got = check_stream(ctx, at_block(s, block))
        if first is None:
            first = got
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, got)), block


# --- the host form -----------------------------------------------------------------------------------
def named(streams, name):
    return next(s for s in streams if s.name == name)


@pytest.mark.parametrize("s", [named(Wc.windows(), f"window_overwrites/{Wc.CAP}"),
                               named(Wc.wide(), f"straddle_0/{Wc.DEFAULT_CAP}")], ids=lambda s: s.name)
def test_host_form_equals_the_device_form(ctx, s):
    p = s.expected()
    dev = check_stream(ctx, s)
    for pinned in (False, True):
        ctx.set_option("cut_block", s.block)
        ctx.set_option("cut_walk_cap", s.cap)
        ents, src, segs = ctx.db_write_plan(s.g.keys, s.g.vals, s.g.cmds, s.limit, s.tomb_off, pinned=pinned)
        assert ctx.get_stat("cut_long") == p.long_count(s.cap)
        assert ents.tobytes() == dev[0].tobytes() and src.tolist() == p.src and segs.tobytes() == dev[2].tobytes()
        assert s.entries_of(ents) == p.entries
