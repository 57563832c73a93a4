"""The write plan's cases (write_cases.py) on the CPU: the restatement agrees
with itself -- a segment's mem_bytes is the sum of klen + vlen over its
entries, a closed segment's is at least the limit and its last command an
Insert --, and every stream reaches the edge it is named for.  No GPU and
nothing of the library's plan is used here."""
import pytest

import write_cases as Wc
from lsm_storage_engine_amd import wal

ALL = Wc.smallest() + Wc.rule() + Wc.placement() + [Wc.sized(n, Wc.CAP) for n in (63, 257, 1025)]
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
