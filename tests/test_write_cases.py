"""The write plan's cases (write_cases.py) on the CPU: the restatement agrees
with itself -- a segment's mem_bytes is the sum of klen + vlen over its
entries, a closed segment's is at least the limit and its last command an
Insert --, and every stream reaches the edge it is named for.  No GPU and
nothing of the library's plan is used here."""
import pytest

import write_cases as Wc
from lsm_storage_engine_amd import wal

ALL = Wc.smallest() + Wc.rule() + Wc.placement() + [Wc.sized(n, Wc.CAP) for n in (63, 257, 1025)] + Wc.windows() + \
    Wc.wide()
BY_NAME = {s.name: s for s in ALL}


@pytest.mark.parametrize("s", ALL, ids=lambda s: s.name)
def test_plan_is_consistent(s):
    p, recs = s.expected(), s.g.records()
    assert len(p.segs) == p.nflush + 1 and sum(p.lens) == len(s) and p.segs[0][:2] == (0, 0)
    for g, (first_cmd, first_ent, nbytes) in enumerate(p.segs):
        ents = p.seg_entries(g)
        assert nbytes == sum(len(k) + len(v) for k, v in ents)
        assert all(first_cmd <= c < first_cmd + p.lens[g] for c in p.src[first_ent:first_ent + len(ents)])
        assert [k for k, _ in ents] == sorted({r.key for r in recs[first_cmd:first_cmd + p.lens[g]]})
        if g < p.nflush:
            assert nbytes >= s.limit and p.lens[g] >= 1
            assert isinstance(recs[first_cmd + p.lens[g] - 1], wal.Insert)
    # a delete that is a last writer is an entry with the value [0]
    for (k, v), c in zip(p.entries, p.src):
        assert recs[c].key == k and (v == recs[c].val if isinstance(recs[c], wal.Insert) else v == Wc.DELETED)


def lens(name):
    return BY_NAME[name].expected().lens


def test_smallest_reach_their_edges():
    assert lens("n0") == [0] and lens("n1_insert") == [1] and lens("n1_delete") == [1]
    assert lens("one_below_limit") == [1] and lens("one_at_limit") == [1, 0] and lens("one_above_limit") == [1, 0]
    assert lens("only_deletes") == [4] and lens("only_deletes_limit_0") == [3]
    assert lens("limit_0_deletes_between") == [1, 3, 1, 2]  # a cut behind every Insert, none behind a delete
    assert lens("cut_on_last") == [4, 0] and lens("no_cut") == [7] == lens("no_cut_small")
    p = BY_NAME["no_cut"].expected()  # the single memtable, tombstones kept
    assert p.entries == [(b"a", b"333"), (b"b", b"\0"), (b"c", b"\0"), (b"d", b"\0")] and p.segs == [(0, 0, 10)]


def test_rule_streams_reach_their_edges():
    assert lens("delete_past_then_shrink") == [6] and BY_NAME["delete_past_then_shrink"].expected().segs[0][2] == 11
    p = BY_NAME["delete_past_then_keep"].expected()
    assert p.lens == [4, 1] and p.segs[0][2] == 17
    assert lens("overwrite_counts_once") == [4, 1]
    assert lens("prev_last_of_previous") == [1, 2, 1]
    assert lens("prev_first_of_segment") == [1, 4, 1]
    p = BY_NAME["big_then_small"].expected()
    assert p.lens == [5, 1] and p.segs[0][2] == 25
    p = BY_NAME["delete_last_writer"].expected()
    assert p.lens == [4, 1] and (b"k", b"\0") in p.seg_entries(0) and p.src[0] == 2
    p = BY_NAME["delete_then_insert"].expected()
    assert p.lens == [4, 2] and (b"k", b"new") in p.seg_entries(0) and (b"k", b"again") in p.seg_entries(1)


def test_placement_streams_reach_their_edges():
    B = Wc.BLOCK
    for cap in (Wc.DEFAULT_CAP, Wc.CAP):
        assert lens(f"end_at_block-1/{cap}")[0] == B and lens(f"end_at_block/{cap}")[0] == B + 1
        assert lens(f"end_at_block+1/{cap}")[0] == B + 2
        p = BY_NAME[f"spans_blocks/{cap}"].expected()
        starts = {s[0] for s in p.segs}
        assert not starts & set(range(B, 2 * B)) and not starts & set(range(3 * B, 5 * B))  # blocks no chain enters
        assert [len(BY_NAME[f"n_block_multiple{d}/{cap}"]) for d in ("-1", "", "+1")] == [2 * B - 1, 2 * B, 2 * B + 1]
        assert lens(f"walks_1_and_300/{cap}")[:4] == [1, 300, 1, 300]
        assert BY_NAME[f"spans_blocks/{cap}"].expected().long_count(cap) == (0 if cap > 300 else 2)
    s = BY_NAME["around_cap_64"]
    assert s.expected().lens == [63, 64, 65, 5, 64, 66, 64] and s.expected().long_count(s.cap) == 2
    s = BY_NAME["around_cap_4"]
    assert s.expected().lens == [3, 4, 5, 2, 4, 6, 4] and s.expected().long_count(s.cap) == 2
    assert BY_NAME["open_above_cap_4"].expected().long_count(Wc.CAP_SMALL) == 1  # the open segment itself
    s = BY_NAME["long_inside_block"]
    assert s.expected().lens[:3] == [2, 20, 3] and sum(s.expected().lens[:6]) < Wc.BLOCK
    assert s.expected().long_count(s.cap) == 2
    assert BY_NAME["cap_1"].expected().long_count(1) == 3


def test_sized_streams_cut_and_hold_deletes():
    for n in (63, 257, 1025):
        p = BY_NAME[f"sized_{n}/{Wc.CAP}"].expected()
        assert p.nflush >= 3 and any(v == Wc.DELETED for _, v in p.entries)
        assert len(p.entries) < n  # keys are overwritten inside a segment


def cuts(name):
    """The commands that closed a memtable."""
    p = BY_NAME[name].expected()
    return [p.segs[g][0] + p.lens[g] - 1 for g in range(p.nflush)]


def test_window_streams_reach_their_edges():
    W, E = Wc.W, Wc.E
    assert len(Wc.windows()) == 2 * (len(Wc.WINDOW_LENGTHS) + 5)
    for cap in (Wc.CAP_SMALL, Wc.CAP):
        small = 2 if cap == Wc.CAP_SMALL else 0  # the segment of 5 commands is LONG at cap 4; the open one of 3 is not
        for ln in Wc.WINDOW_LENGTHS:
            s = BY_NAME[f"long_len_{ln}/{cap}"]
            assert (s.cap, s.block, s.limit) == (cap, Wc.BLOCK, Wc.TW)
            p = s.expected()
            assert p.lens == [E, ln, 5, 2, 3] and p.segs[1][0] == E and cuts(s.name)[1] == E + ln - 1
            assert p.long_count(cap) == 1 + small // 2
        # the cut's lane in its window, and the window
        assert [((ln - 1) % W, (ln - 1) // W) for ln in Wc.WINDOW_LENGTHS] == \
            [(1022, 0), (1023, 0), (0, 1), (1, 1), (1022, 1), (1023, 1), (0, 2), (0, 3)]
        s = BY_NAME[f"long_back_to_back/{cap}"]
        p = s.expected()
        assert p.lens == [E, 1500, 1024, 2049, 1100] and p.long_count(cap) == 4 and len(s) % W != 0
        assert cuts(s.name) == [E - 1, E + 1499, E + 2523, E + 4572]
        assert W < p.lens[-1] < 2 * W  # the open memtable ends inside its second window
        s = BY_NAME[f"long_cut_on_last/{cap}"]
        p = s.expected()
        assert p.lens == [E, 1030, 0] and cuts(s.name)[-1] == len(s) - 1 and p.long_count(cap) == 1
        assert p.segs[-1] == (len(s), len(p.entries), 0) and (1030 - 1) // W == 1

        s = BY_NAME[f"window_overwrites/{cap}"]
        p, recs = s.expected(), s.g.records()
        assert p.lens == [E, Wc.OVERWRITES_CUT - E + 1, 5] and cuts(s.name) == [E - 1, Wc.OVERWRITES_CUT]
        assert p.long_count(cap) == 1 + small // 2 and s.limit == Wc.OVERWRITES_LIMIT
        t = Wc.bytes_trace(recs, E)
        key = [r.key for r in recs]
        # (a) the key of command E + 1500 was last written before E: its pair is added whole
        assert key[E + 1500] == key[1] == b"PREV" and key.index(b"PREV", E) == E + 1500
        assert t[1500] - t[1499] == len(recs[E + 1500].key) + len(recs[E + 1500].val) == 5
        # (b) a of 5000 at E + 10, taken away in window 1, whose running total is negative from there to its last
        # lane but one (bytes passes the limit on the last lane, (c), so the whole window's total cannot be negative;
        # window_negative_total's is)
        assert t[10] - t[9] == 5000 and key[E + 10] == key[E + 1030] and t[1030] - t[1029] == 4 - 5000
        assert all(t[j] - t[W - 1] < 0 for j in range(1030, 2 * W - 1)) and t[2 * W - 2] - t[W - 1] == -907
        # (c) bytes >= limit first holds after the delete on window 1's last lane
        assert max(t[:2 * W - 1]) < s.limit <= t[2 * W - 1] and isinstance(recs[E + 2 * W - 1], wal.Remove)
        # (d) the Insert behind it overwrites a large value: under the limit again
        assert isinstance(recs[E + 2 * W], wal.Insert) and t[2 * W] == t[2 * W - 1] - 1000 < s.limit
        # (e) the cut, hundreds of commands on in window 2
        first = next(j for j in range(2 * W, len(t)) if isinstance(recs[E + j], wal.Insert) and t[j] >= s.limit)
        assert E + first == Wc.OVERWRITES_CUT and first // W == 2 and first - 2 * W == 204
        assert p.segs[1] == (E, E, t[first])
        assert key[Wc.OVERWRITES_CUT + 2] == key[E + 10]  # a key of the memtable before, written again behind the cut

        s = BY_NAME[f"window_negative_total/{cap}"]
        p, recs = s.expected(), s.g.records()
        t = Wc.bytes_trace(recs, E)
        assert p.lens == [E, Wc.NEGATIVE_CUT - E + 1, 5] and cuts(s.name) == [E - 1, Wc.NEGATIVE_CUT]
        assert t[2 * W - 1] - t[W - 1] == -904 and max(t[:Wc.NEGATIVE_CUT - E]) < s.limit <= t[Wc.NEGATIVE_CUT - E]
        assert (Wc.NEGATIVE_CUT - E) // W == 2 and p.long_count(cap) == 1 + small // 2

        s = BY_NAME[f"long_random/{cap}"]
        p = s.expected()
        assert s.limit == Wc.LONG_RANDOM_LIMIT and len(s) == 20000
        assert p.lens == [2900, 2845, 2862, 2922, 2793, 2982, 2696]
        assert sum(1 for ln in p.lens[:-1] if ln > W) >= 3 and sum(1 for ln in p.lens[:-1] if ln > 2 * W) >= 1
        assert any(v == Wc.DELETED for _, v in p.entries) and len(p.entries) < len(s)


def test_wide_streams_reach_their_edges():
    B, CAP = Wc.DEFAULT_BLOCK, Wc.DEFAULT_CAP
    assert all(s.block == B and len(s) > 2 * B for s in Wc.wide() if s.name != "many_entries_in_block")
    assert Wc.WIDE_BLOCKS == (8192, 8191, 4097, 2048, 1025, 1024, 1000, 65)
    s = BY_NAME["hops_ones"]
    p = s.expected()
    assert len(s) == 2 * B + 77 and p.lens == [1] * len(s) + [0] and p.nflush == len(s) and p.long_count(s.cap) == 0
    for cap in (CAP, Wc.CAP):
        s = BY_NAME[f"hops_mixed/{cap}"]
        p = s.expected()
        assert len(s) == 2 * B + 77 and s.limit == 64 and s.cap == cap and p.nflush == 3658 and max(p.lens) <= 64
        assert len(set(p.lens)) > 5 and any(v == Wc.DELETED for _, v in p.entries) and len(p.entries) < len(s)
        for d in (-1, 0, 1):
            s = BY_NAME[f"straddle_{d:+d}/{cap}" if d else f"straddle_0/{cap}"]
            p = s.expected()
            assert s.cap == cap and B + d in cuts(s.name) and p.lens[160] == B + d + 1 - 8000
            assert p.segs[160][0] == 8000 and p.lens[:160] == [50] * 160 and p.lens[161:163] == [3, 5]
            assert p.long_count(cap) == (0 if cap == CAP else 1)
    for cap in (CAP, 4 * B):
        s = BY_NAME[f"covers_a_block/{cap}"]
        p = s.expected()
        assert s.cap == cap and p.lens == [100, 2 * B + 200, 5, 3, 7, 20] and p.segs[1][0] == 100
        assert not {x[0] for x in p.segs} & set(range(B, 2 * B))  # block 1 is entered by no chain
        assert cuts(s.name)[1] == 100 + 2 * B + 199 and cuts(s.name)[1] // B == 2
        assert p.long_count(cap) == (1 if cap == CAP else 0) and -(-p.lens[1] // Wc.W) == 17
    s = BY_NAME["around_cap_4096"]
    assert (s.cap, s.block) == (CAP, B) and s.expected().lens == [4095, 4096, 4097, 5, 4096, 4098, 4096]
    assert s.expected().long_count(s.cap) == 2
    s = BY_NAME["many_entries_in_block"]
    p = s.expected()
    assert s.cap == 1 and len(s) == B + 100 and set(p.lens[:-1]) == {2, 3} and p.lens[-1] == 2
    assert p.long_count(1) == len(p.segs) == 3317
    assert sum(1 for x in p.segs if x[0] < B) > 256


def test_big_at_32_kib_closes_memtables_longer_than_a_window():
    p = Wc.big(Wc.BIG_WINDOW_LIMIT).expected()
    assert sum(1 for ln in p.lens[:-1] if ln > Wc.W) >= 10 and Wc.BIG_WINDOW_LIMIT not in Wc.BIG_LIMITS
    assert p.long_count(Wc.CAP) == len(p.segs)
