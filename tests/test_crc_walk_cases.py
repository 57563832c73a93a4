"""The layouts of tests/crc_walk_cases.py hold what test_gpu_crc_walk_edges.py
relies on: full coverage of the spaces they claim, every record inside its
buffer, and the walking kernel's record map (tools/walk_sim.py, the lane-level
CPU model of crc32_walk_kernel) correct on every one of them.  CPU-only."""
import os
import sys
import zlib

import numpy as np
import pytest

import crc_walk_cases as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import walk_sim  # noqa: E402

NW = (1, 7, 4096)  # waves: one run, uneven cuts, 256 CUs x 16 waves


@pytest.fixture(scope="module")
def lanes():
    return W.lane_matrix()


def _inside(off, ln, nbytes):
    off, ln = off.astype(np.int64), ln.astype(np.int64)
    return len(off) == len(ln) and (off >= 0).all() and (off + ln + W.SLACK <= nbytes).all()


@pytest.mark.parametrize("base_ptr", [0x7F0000200000, 0x7F0000200003, 0x7F0000200FFF])
def test_page_matrix_holds_every_length_and_distance_once(base_ptr):
    off, ln, meta = W.page_matrix(base_ptr)
    assert off.dtype == np.uint64 and ln.dtype == np.uint32
    assert len(off) == 384 * 132 == 50688
    pairs = set(zip(meta["L"].tolist(), meta["D"].tolist()))
    assert pairs == {(L, D) for L in range(1, 385) for D in range(132)} and len(pairs) == len(off)
    assert np.array_equal(ln, meta["L"])
    A = off.astype(np.int64) + base_ptr
    assert np.array_equal(A % W.PAGE, meta["D"])        # each record's absolute start is at a page + D
    assert len(np.unique(A // W.PAGE)) == 64 and A.min() // W.PAGE > base_ptr // W.PAGE
    assert _inside(off, ln, meta["nbytes"]) and meta["nbytes"] < 320 << 10
    assert np.array_equal(np.sort(meta["perm"]), np.arange(len(off))) and (meta["perm"] != np.arange(len(off))).any()
    # the states of seg_issue<false> the matrix is there for
    lead, sh, m = W.load_shape(base_ptr, off, ln)
    first = ln.astype(np.int64) <= 128
    assert set(lead[first].tolist()) == set(range(0, 128))
    assert set(m.tolist()) == set(range(0, 33))
    # every reachable (lead, sh, m): the boundary lies at a dword of (p, B], so m <= (sh + lead) / 4
    assert set(zip(lead[first].tolist(), sh[first].tolist(), m[first].tolist())) \
        == {(a, b, c) for a in range(128) for b in range(4) for c in range((a + b) // 4 + 1)}
    # behind a first segment of every shape: a second and a third segment (full, never moved)
    more = ~first
    assert set(zip(lead[more].tolist(), sh[more].tolist(), m[more].tolist())) \
        == {(a, b, c) for a in range(128) for b in range(4) for c in range((a + b) // 4 + 1)}
    # D_32 is the dword behind the window (sh != 0 and m == 0) and a dword inside it, for every lead
    d32 = (sh != 0) & (m == 0)
    assert set(lead[first & d32].tolist()) == set(lead[first & ~d32].tolist()) == set(range(128))
    # D >= 128: the window starts on the record's page, never moved
    assert (m[meta["D"] >= 128] == 0).all() and (m[(meta["D"] == 0)] > 0).sum() > 0


def test_load_shape_is_the_kernels_arithmetic():
    """load_shape against a scalar transcription of seg_issue<false>."""
    rng = np.random.default_rng(3)
    base = 0x7F0000200003
    off = rng.integers(0, 1 << 20, 3000).astype(np.uint64)
    ln = rng.integers(1, 700, 3000).astype(np.uint32)
    lead, sh, m = W.load_shape(base, off, ln)
    for i in range(len(off)):
        rec_len = int(ln[i])
        k = (rec_len + 127) // 128 - 1
        E = int(off[i]) + rec_len - 128 * k
        seglen = rec_len - 128 * k
        ld = 128 - seglen
        s0 = base + E - 128
        s = s0 & 3
        p = s0 - s
        pg = (p + s + ld) & ~4095
        mm = (pg - p) >> 2 if (ld < 128 and pg > p) else 0
        assert (ld, s, mm) == (lead[i], sh[i], m[i]) and 0 <= mm <= 32


def test_lane_matrix_hits_every_lane_and_segment_count(lanes):
    off, ln, meta = lanes
    assert off.dtype == np.uint64 and ln.dtype == np.uint32
    ns, pre = W.nseg(ln), W.seg_prefix(ln)
    pr = meta["probe"]
    assert len(pr) == 64 * 136 == 8704
    hit = set(zip((pre[pr] % 64).tolist(), ns[pr].tolist()))
    assert hit == {(s, k) for s in W.LANE_S for k in W.LANE_K} and len(hit) == len(pr)
    assert np.array_equal(pre[pr] % 64, meta["s"]) and np.array_equal(ns[pr], meta["k"])
    even = meta["s"] % 2 == 0
    assert (ln[pr][even] == 128 * meta["k"][even]).all() and (ln[pr][~even] == 128 * (meta["k"][~even] - 1) + 1).all()
    sums = W.superblock_sums(ln)
    assert len(sums) == (len(ln) + 255) // 256 and (sums % 64 == 0).all()
    full_pads = np.arange(255, len(ln), 256)
    assert np.array_equal(meta["pad"][:len(full_pads)], full_pads) and len(meta["pad"]) <= len(full_pads) + 1
    assert not set(meta["pad"].tolist()) & set(pr.tolist())
    assert (ln == 0).sum() > 100                               # empty records occupy lanes too
    assert ln.max() == 257 * 128 == 32896
    assert _inside(off, ln, meta["nbytes"])
    assert (np.diff(off.astype(np.int64)) < 0).any()           # unsorted
    assert not W.stream_eligible(off, ln)
    # probes that end inside their tile, exactly on lane 63, and carry over 1, 2, 3 and 4 tiles
    end = meta["s"] + meta["k"] - 1
    assert (end < 63).any() and set(np.unique(end // 64).tolist()) == {0, 1, 2, 3, 4}
    assert set(meta["s"][end == 63].tolist()) == set(range(64))
    assert {63, 127, 191, 255} <= set(end.tolist())


def test_window_cases_cover_every_phase_and_burst():
    cases = W.window_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) == 64 * 11 + 6 + 14
    by = {c[0]: c for c in cases}
    seen_len = set()
    for p in W.WIN_P:
        for b in W.WIN_B:
            _, off, ln = by[f"p{p}_b{b}"]
            ns = W.nseg(ln)
            lead = 1 if p else 0
            assert len(ln) == lead + b + 1
            assert (ns[0] == p if p else True) and (ns[lead:lead + b] == 1).all() and ns[-1] == W.WIN_TAIL
            assert (ln[lead:lead + b] <= 128).all()
            seen_len |= set(ln[lead:lead + b].tolist())
            assert W.seg_prefix(ln)[lead] == p                 # the burst starts on lane p
            assert _inside(off, ln, W.WIN_BLOB)
    assert seen_len == set(range(0, 129))
    for n in W.EMPTY_N:
        _, off, ln = by[f"empty_{n}"]
        assert len(ln) == n and (ln == 0).all() and _inside(off, ln, W.WIN_BLOB) and not W.stream_eligible(off, ln)
    for n in W.MIXED_N:
        _, off, ln = by[f"mixed_{n}"]
        assert len(ln) == n and ln.max() <= 700 and _inside(off, ln, W.WIN_BLOB)
        assert W.stream_eligible(off, ln) == (ln[0] != 0)
    elig = [W.stream_eligible(off, ln) for _, off, ln in cases]
    assert 0 < sum(elig) < 40                                  # both kinds: most batches are declined


def test_stream_eligible_is_the_checks_rule():
    E = W.stream_eligible
    u64, u32 = (lambda *a: np.array(a, dtype=np.uint64)), (lambda *a: np.array(a, dtype=np.uint32))
    assert E(u64(5, 15, 15 + 64 + 20), u32(10, 20, 7))         # packed, then a gap of exactly 64
    assert not E(u64(5, 15, 15 + 65 + 20), u32(10, 20, 7))     # gap 65
    assert not E(u64(5, 14), u32(10, 20))                      # overlap
    assert not E(u64(15, 5), u32(10, 5))                       # unsorted
    assert not E(u64(5, 15), u32(0, 20))                       # empty first
    assert E(u64(5, 15, 15), u32(10, 0, 3))                    # empty, packed
    assert not E(u64(5, 16, 16), u32(10, 0, 3))                # empty behind a gap


def test_scale_and_fixed_layouts():
    for n in W.SCALE_N:
        off, ln = W.scale_batch(n)
        assert len(off) == len(ln) == n and off.dtype == np.uint64 and ln.dtype == np.uint32
        assert _inside(off, ln, W.SCALE_BYTES) and ln.max() <= 700
        assert 0.89 < (ln <= 96).mean() < 0.91 and (ln == 0).any()
        assert not W.stream_eligible(off[:1000], ln[:1000])
        nsb = (n + 255) // 256
        assert (nsb + 1023) // 1024 == {262_145: 2, 4_194_309: 17}[n]   # scan_phase2's C
    assert (4_194_309 + 255) // 256 > 16 * 2 * 512                       # walk_phase1 grid-strides up to 512 CUs
    assert 4_194_309 > 8192 * 256                                        # so does crc32_compare_kernel
    fl = W.fixed_lengths()
    assert len(fl) == len(set(fl)) == 131 + 4 + 4 + 4 + 3 and set(range(1, 132)) <= set(fl)
    assert {255, 258, 383, 386, 1023, 1026, 8191, 8193} <= set(fl)
    assert {64 % ((L + 127) // 128) != 0 for L in fl} == {False, True}   # with and without straddling records
    for shift in W.FIXED_SHIFTS:
        start = shift + np.arange(W.FIXED_N) * W.FIXED_STRIDE
        assert len(np.unique(start % 4096)) == 4096
        assert start[-1] + max(fl) + W.SLACK <= W.fixed_nbytes()
    assert W.fixed_nbytes() < 18 << 20


def test_mismatch_report_and_zlib_reference():
    data = np.arange(1000, dtype=np.uint32).view(np.uint8)
    off, ln = np.array([0, 5, 300], dtype=np.uint64), np.array([0, 200, 129], dtype=np.uint32)
    want = W.zlib_batch(data, off, ln)
    assert want[0] == 0 and want[1] == zlib.crc32(data[5:205].tobytes())
    bad, msg = W.mismatches(want, want, off, ln)
    assert len(bad) == 0
    got = want.copy()
    got[2] ^= 1
    bad, msg = W.mismatches(got, want, off, ln)
    assert bad.tolist() == [2] and "(2, 300, 129, 3, 2," in msg      # lane 3: segments 1 + 2 in front


@pytest.mark.parametrize("nw", NW)
def test_walk_map_on_lane_matrix(lanes, nw):
    _, ln, _ = lanes
    assert walk_sim.simulate(ln.astype(np.int64), nw) == W.nseg(ln).sum()


@pytest.mark.parametrize("nw", NW)
def test_walk_map_on_window_cases(nw):
    """Every batch for nw = 1 and 7.  For nw = 4096 the simulator's loop over
    the (mostly empty) waves takes 14 s over all 724 batches, so there it runs
    on every batch of more than one superblock -- the only ones a cut can
    fall inside -- and on a seeded tenth of the others."""
    cases = W.window_cases()
    if nw == 4096:
        keep = np.random.default_rng(1).random(len(cases)) < 0.1
        cases = [c for c, k in zip(cases, keep) if k or len(c[2]) > W.WALK_SB]
        assert 150 < len(cases) < 300
    for name, _, ln in cases:
        assert walk_sim.simulate(ln.astype(np.int64), nw) == W.nseg(ln).sum(), name


@pytest.mark.parametrize("nw", NW)
def test_walk_map_on_scale_lengths(nw):
    _, ln = W.scale_batch(W.SCALE_N[0])
    assert walk_sim.simulate(ln.astype(np.int64), nw) == W.nseg(ln).sum()
