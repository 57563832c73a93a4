"""Layouts for the walking CRC kernel's edge tests (test_gpu_crc_walk_edges.py).

crc32_walk_kernel (lsmck_crc32.hip) branches on two things.  Its load path
(seg_issue<false> / seg_finish<false>) branches on a record's first-segment
length (lead), on the byte alignment of its end (sh) and on whether a 4 KiB
boundary of the *absolute* address lies between the load window's start and
the record's first byte (the window then moves up by m dwords).  Its record
map branches on the lane a record starts on, on its segment count relative to
the 64 lanes of a tile, and on where tile boundaries fall inside the ring of
three 64-record windows.  Each layout below walks one of these spaces
completely; payload bytes come from O.gen_stream, so a layout is only
(off uint64[], len uint32[]) and what the CPU test checks about it.

Nothing in this module needs a GPU: tests/test_crc_walk_cases.py checks it.
"""
import zlib

import numpy as np

PAGE = 4096
SEG = 128          # bytes per segment
TILE = 64          # segments per tile (lanes)
WALK_SB = 256      # records per superblock (lsmck_crc32.hip)
SLACK = 4096       # bytes kept after the last record's end in every payload buffer
CANARY = 0xA5A5A5A5  # every `out` buffer is pre-filled with it: an unwritten CRC shows
STREAM_MAX_GAP = 64  # lsmck_crc32.hip: the stream kernel's largest gap between two records


def nseg(ln):
    """Segments a record owns in the walking kernel: max(1, ceil(len / 128))."""
    ln = np.asarray(ln).astype(np.int64)
    return np.where(ln == 0, 1, (ln + SEG - 1) // SEG)


def seg_prefix(ln):
    """Global index of every record's first segment (exclusive prefix of nseg)."""
    ns = nseg(ln)
    return np.cumsum(ns) - ns


def superblock_sums(ln):
    """Segment total of every superblock of WALK_SB records."""
    ns = nseg(ln)
    return np.add.reduceat(ns, np.arange(0, len(ns), WALK_SB)) if len(ns) else np.zeros(0, np.int64)


def stream_eligible(off, ln):
    """Whether stream_check (lsmck_crc32.hip) lets the stream kernel take a
    caller's batch: sorted, not overlapping, gaps of at most STREAM_MAX_GAP
    bytes, no empty record first or behind a gap.  A batch it declines goes to
    the walking kernel under the default dispatch."""
    off = np.asarray(off, dtype=np.uint64)
    ln = np.asarray(ln, dtype=np.uint32).astype(np.uint64)
    if len(ln) == 0 or ln[0] == 0:
        return False
    end, nxt = off[:-1] + ln[:-1], off[1:]
    bad = (nxt < end) | (nxt > end + np.uint64(STREAM_MAX_GAP)) | ((ln[1:] == 0) & (nxt != end))
    return not bad.any()


def zlib_batch(data, off, ln):
    """zlib.crc32 of data[off[i] : off[i] + ln[i]) per record: the independent reference."""
    mv = memoryview(np.ascontiguousarray(data, dtype=np.uint8)).cast("B")
    return np.array([zlib.crc32(mv[o:o + l]) for o, l in zip(np.asarray(off).tolist(), np.asarray(ln).tolist())],
                    dtype=np.uint32)


def mismatches(got, want, off, ln, limit=8):
    """Indices where two CRC arrays differ, and a readable list of the first
    few with each record's off, len, lane (its first segment's index mod 64:
    the lane it starts on when every wave's run starts on a multiple of 64
    segments, as in lane_matrix) and segment count."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    ns, pre = nseg(ln), seg_prefix(ln)
    head = [(int(i), int(off[i]), int(ln[i]), int(pre[i] % TILE), int(ns[i]), "%08x" % got[i], "%08x" % want[i])
            for i in bad[:limit]]
    return bad, f"{len(bad)} of {len(want)} CRCs differ; first (index, off, len, lane, nseg, got, want): {head}"


# --- (a) the segment path: every (length, distance behind a page boundary) ---------
PAGE_L = range(1, 385)     # 1..128: every lead; 129..384: non-first segments behind each first-segment shape
PAGE_D = range(0, 132)     # D >= 128: m = 0; smaller D: every m = 1..32; L + D: every end alignment
PAGE_NPAGES = 64


def page_matrix(base_ptr, seed=21):
    """One record per (L, D) of PAGE_L x PAGE_D, L-major: L bytes starting D
    bytes after a 4 KiB boundary of the absolute address base_ptr + off.
    Record i lies on page 1 + i % 64 of the pages of the buffer at base_ptr
    (page 0: the one holding, or starting at, base_ptr), so the records
    overlap.  Returns (off, ln, meta): meta["L"], meta["D"] per record,
    meta["perm"] a seeded shuffle of the records, meta["nbytes"] the payload
    size including SLACK."""
    L, D = np.meshgrid(np.arange(PAGE_L.start, PAGE_L.stop), np.arange(PAGE_D.start, PAGE_D.stop), indexing="ij")
    L, D = L.ravel().astype(np.int64), D.ravel().astype(np.int64)
    first = (-int(base_ptr)) % PAGE               # offset of the first page boundary at or after base_ptr
    page = 1 + np.arange(len(L), dtype=np.int64) % PAGE_NPAGES
    off = (first + page * PAGE + D).astype(np.uint64)
    nbytes = first + (PAGE_NPAGES + 1) * PAGE + PAGE_D.stop + PAGE_L.stop + SLACK
    perm = np.random.default_rng(seed).permutation(len(L))
    return off, L.astype(np.uint32), {"L": L, "D": D, "perm": perm, "nbytes": int(nbytes)}


def load_shape(base_ptr, off, ln):
    """(lead, sh, m) of every record's first segment as seg_issue<false>
    computes them: lead = 128 - first-segment length, sh = the stream start's
    byte alignment ((E - 128) & 3), m = dwords the load window moves up to the
    start of the record's page (0: no boundary between window and record)."""
    A = np.asarray(off).astype(np.int64) + int(base_ptr)
    ln = np.asarray(ln).astype(np.int64)
    first_len = ln - SEG * (nseg(ln) - 1)
    lead = SEG - first_len
    s0 = A + first_len - SEG                       # E - 128 of the first segment
    sh = s0 & 3
    p = s0 - sh
    pg = (p + sh + lead) & ~np.int64(PAGE - 1)     # the page of the record's first byte
    m = np.where((lead < SEG) & (pg > p), (pg - p) >> 2, 0)
    return lead, sh, m


# --- (b) the record map: every (start lane, segment count) ---------------------------
LANE_S = range(0, TILE)
LANE_K = tuple(range(1, 131)) + (191, 192, 193, 255, 256, 257)
LANE_BLOB = 1 << 20
SPLIT_LENS = (0, 1, 127, 128)  # one-segment filler records, empty ones included


def lane_matrix(seed=22):
    """For every start lane s of LANE_S and segment count k of LANE_K one
    probe record of k segments whose first segment is segment s (mod 64) of
    the batch: a filler record in front of it brings the running segment
    count to s (mod 64); every fourth filler is f one-segment records
    instead (lengths cycling through SPLIT_LENS).  Every record with index
    255 (mod 256) is a pad record that rounds its superblock's segment sum
    up to a multiple of 64, and so does the last record: a wave's run is a
    whole number of superblocks, so every run starts on lane 0 and a
    record's lane does not depend on where the cuts fall.  A probe is 128k
    bytes long for even s and 128(k-1)+1 for odd s.  Offsets are seeded
    random positions in a blob of LANE_BLOB bytes (overlapping, unsorted).
    Returns (off, ln, meta): meta["probe"] the probes' record indices,
    meta["s"], meta["k"] per probe, meta["pad"] the pad records' indices,
    meta["nbytes"]."""
    lens, probe, ps, pk, pads = [], [], [], [], []
    cur = 0      # segments so far
    sb = 0       # segments so far in the current superblock
    nfill = 0
    nsplit = 0

    def emit(length):
        nonlocal cur, sb
        k = 1 if length == 0 else (length + SEG - 1) // SEG
        lens.append(length)
        cur += k
        sb += k
        if len(lens) % WALK_SB == 0:
            sb = 0

    def pad_if_due():
        if len(lens) % WALK_SB == WALK_SB - 1:
            k = TILE - sb % TILE                     # 1..64 segments
            pads.append(len(lens))
            emit(SEG * k - (len(pads) * 29) % SEG)   # any length of k segments
    for s in LANE_S:
        for k in LANE_K:
            counted = split = False
            while True:  # (a pad record in the filler's way resets the count: fill again behind it)
                pad_if_due()
                f = (s - cur) % TILE
                if f == 0:
                    break
                if not counted:
                    counted = True
                    nfill += 1
                    split = nfill % 4 == 0
                if split:
                    emit(SPLIT_LENS[nsplit % len(SPLIT_LENS)])
                    nsplit += 1
                else:
                    emit(SEG * (f - 1) + 1 + (nfill * 37) % SEG)
            probe.append(len(lens))
            ps.append(s)
            pk.append(k)
            emit(SEG * k if s % 2 == 0 else SEG * (k - 1) + 1)
    if sb % TILE:
        pads.append(len(lens))
        emit(SEG * (TILE - sb % TILE))
    ln = np.array(lens, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    off = (rng.random(len(ln)) * (LANE_BLOB - SLACK - ln.astype(np.int64))).astype(np.uint64)
    meta = {"probe": np.array(probe), "s": np.array(ps), "k": np.array(pk), "pad": np.array(pads),
            "nbytes": LANE_BLOB}
    return off, ln, meta


# --- (c) the window ring and the batch-size edges ------------------------------------
WIN_P = range(0, TILE)
WIN_B = (63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 300)
WIN_TAIL = 70
EMPTY_N = (1, 64, 65, 256, 257, 1000)
MIXED_N = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
WIN_BLOB = 1 << 20


def window_cases(seed=23):
    """Small batches over one blob of WIN_BLOB bytes, as a list of
    (name, off, ln):
      * for every phase p of WIN_P and burst length b of WIN_B: one record of
        p segments (none for p = 0), b one-segment records (lengths cycling
        through 0..128) and one record of WIN_TAIL segments -- the burst's 64-
        record windows begin at every lane of a tile, and the tile boundaries
        at every place in the ring; seeded random offsets (overlapping,
        unsorted);
      * batches of only empty records, n of EMPTY_N, random offsets;
      * batches of n of MIXED_N records of 0..700 bytes, packed back to back
        from offset 1 (the stream kernel takes them under the default
        dispatch unless the first record is empty)."""
    rng = np.random.default_rng(seed)
    cases = []

    def scattered(ln):
        ln = np.asarray(ln, dtype=np.uint32)
        off = (rng.random(len(ln)) * (WIN_BLOB - SLACK - ln.astype(np.int64))).astype(np.uint64)
        return off, ln
    cyc = 0
    for p in WIN_P:
        for b in WIN_B:
            ln = [SEG * p - (p * 11 + b) % SEG] if p else []
            ln += [(cyc + i) % (SEG + 1) for i in range(b)]
            cyc += b
            ln.append(SEG * WIN_TAIL - (p + b) % SEG)
            cases.append((f"p{p}_b{b}",) + scattered(ln))
    for n in EMPTY_N:
        cases.append((f"empty_{n}",) + scattered(np.zeros(n, dtype=np.uint32)))
    for n in MIXED_N:
        ln = rng.integers(0, 701, n).astype(np.uint32)
        off = np.uint64(1) + np.concatenate([[0], np.cumsum(ln[:-1].astype(np.uint64))]).astype(np.uint64)
        cases.append((f"mixed_{n}", off, ln))
    return cases


# --- (d) scale: more than one superblock per scan thread, grid-stride loops -----------
SCALE_BYTES = 64 << 20
SCALE_N = (262_145,     # 1,025 superblocks: scan_phase2 C = 2
           4_194_309)   # 16,385 superblocks: C = 17, walk_phase1's grid-stride loop up to 512 CUs,
#                         crc32_compare_kernel's grid-stride loop (n > 8192 * 256)


def scale_batch(n, seed=24):
    """n records inside SCALE_BYTES: 90 % of the lengths in 0..96, 10 % in
    97..700, offsets uniform (overlapping, unsorted).  Returns (off, ln)."""
    rng = np.random.default_rng(seed + n)
    ln = np.where(rng.random(n) < 0.9, rng.integers(0, 97, n), rng.integers(97, 701, n)).astype(np.uint32)
    off = rng.integers(0, SCALE_BYTES - SLACK - 700, n, dtype=np.int64).astype(np.uint64)
    return off, ln


# --- (e) the fixed-record leg of the same load path -------------------------------------
FIXED_STRIDE = 4097   # = 1 (mod 4096): with n >= 4096 records every start offset mod 4096 occurs
FIXED_N = 4300
FIXED_SHIFTS = (0, 1)


def fixed_lengths():
    """Record lengths of the fixed-record leg: every first-segment length and
    the segment counts around 2, 3, 8 and 64 (with and without records that
    straddle 64-segment tiles)."""
    return (list(range(1, 132)) + list(range(255, 259)) + list(range(383, 387)) + list(range(1023, 1027))
            + list(range(8191, 8194)))


def fixed_nbytes():
    """Payload bytes the fixed-record leg needs (the largest shift and length, plus SLACK)."""
    return max(FIXED_SHIFTS) + (FIXED_N - 1) * FIXED_STRIDE + max(fixed_lengths()) + SLACK
