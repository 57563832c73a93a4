"""The walking CRC kernel (crc32_walk_kernel, lsmck_crc32.hip) and the
unaligned segment path it shares with the two-slot fixed kernel
(seg_issue<false> / seg_finish<false>), at every edge their code branches on.
The layouts come from tests/crc_walk_cases.py (checked on the CPU by
tests/test_crc_walk_cases.py); every case runs on device-resident data and is
bit-exact against the oracle (O.crc32_batch / O.crc32_fixed, crc 1.x's
algorithm), one layout per group also against zlib.crc32.  Every `out` buffer
is pre-filled with 0xA5A5A5A5, so an unwritten CRC shows.

The walking kernel is reached by two routes, named in every test:
  walk     crc_stream 0: the walking kernel alone (walk_phase1, scan_phase2,
           crc32_walk_kernel);
  default  the default dispatch (crc_stream 1) on a batch stream_check
           declines (unsorted or overlapping): the check, the declined stream
           kernel, then the walking kernel.
For one batch per group crc_stream 2 (the stream kernel alone) must leave
`out` untouched: the batch really went to the walking kernel.

  1 segment-path matrix   every (length 1..384, distance 0..131 behind a page
                          boundary): every lead, end alignment, window move m
  2 fixed-record leg      the same load path under the two-slot fixed kernel
  3 lane x segment count  every start lane 0..63 x k in 1..130, 191..193,
                          255..257 segments: in-tile ends, lane 63, Horner carry
  4 window ring, n edges  bursts of one-segment records at every tile phase
  5 scale                 scan_phase2 C = 2 and 17, the grid-stride loops of
                          walk_phase1 and crc32_compare_kernel
  6 stores stay in `out`  guard dwords around an `out` at dword offset 1
  7 the comparison fails  when the kernel stores nothing (crc_ablate 3)
"""
import contextlib

import numpy as np
import pytest

import crc_walk_cases as W
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CANARY = np.uint32(W.CANARY)
ROUTES = {"walk": 0, "default": 1}


@contextlib.contextmanager
def _option(ctx, key, value, restore):
    ctx.set_option(key, value)
    try:
        yield
    finally:
        ctx.set_option(key, restore)


def _upload(ctx, arr, shift=0):
    a = np.ascontiguousarray(arr)
    d = ctx.alloc(a.nbytes + shift)
    d.upload(a, offset=shift)
    return d


def _canary_out(ctx, n):
    out = ctx.alloc(4 * n)
    out.upload(np.full(n, CANARY, dtype=np.uint32))
    return out


def _crc(ctx, base_ptr, off, ln, crc_stream):
    """CRCs of the records at base_ptr (a device pointer) under the given
    crc_stream option; unwritten outputs keep the canary."""
    n = len(off)
    d_o, d_l, out = _upload(ctx, off), _upload(ctx, ln), _canary_out(ctx, n)
    try:
        with _option(ctx, "crc_stream", crc_stream, 1):
            ctx.crc32_device(base_ptr, d_o.ptr, d_l.ptr, n, out.ptr)
            ctx.sync()
        return out.download(np.uint32)
    finally:
        for b in (d_o, d_l, out):
            b.free()


def _check(got, want, off, ln, what=""):
    bad, msg = W.mismatches(got, want, off, ln)
    assert len(bad) == 0, f"{what}: {msg}"


def _check_route(ctx, base_ptr, off, ln, want, route, what=""):
    if route == "default":
        assert not W.stream_eligible(off, ln), "the stream kernel would take this batch"
    _check(_crc(ctx, base_ptr, off, ln, ROUTES[route]), want, off, ln, f"{what} [{route}]")


def _declined(ctx, base_ptr, off, ln):
    """The stream kernel alone declines the batch: nothing is written."""
    return (_crc(ctx, base_ptr, off, ln, 2) == CANARY).all()


# --- 1. segment-path matrix -----------------------------------------------------------
SEG_ALLOC = 320 << 10


@pytest.fixture(scope="module", params=[0, 3], ids=["shift0", "shift3"])
def seg(request, ctx):
    """Layout (a) for a payload uploaded `shift` bytes into its allocation:
    the absolute addresses are those of d.ptr + shift."""
    shift = request.param
    d = ctx.alloc(SEG_ALLOC)
    base = d.ptr + shift
    off, ln, meta = W.page_matrix(base)
    assert meta["nbytes"] + shift <= SEG_ALLOC
    data = O.gen_stream(0x5EED0050 + shift, 0, SEG_ALLOC - shift)
    d.upload(data, offset=shift)
    assert np.array_equal((off.astype(np.int64) + base) % 4096, meta["D"])
    want = O.crc32_batch(data, off, ln, threads=8)
    yield {"base": base, "shift": shift, "data": data, "off": off, "ln": ln, "perm": meta["perm"], "want": want}
    d.free()


def test_segment_matrix_in_order(ctx, seg):
    """Route walk.  Matrix order: a tile holds one length at 64 consecutive distances."""
    _check_route(ctx, seg["base"], seg["off"], seg["ln"], seg["want"], "walk", "page matrix")


@pytest.mark.parametrize("route", list(ROUTES))
def test_segment_matrix_shuffled(ctx, seg, route):
    """Routes walk and default.  Shuffled: every lane of a tile holds another
    shape, so the rare window move (m != 0) sits beside unmoved lanes."""
    p = seg["perm"]
    off, ln, want = seg["off"][p], seg["ln"][p], seg["want"][p]
    _check_route(ctx, seg["base"], off, ln, want, route, "shuffled page matrix")
    if route == "default" and seg["shift"] == 3:
        assert _declined(ctx, seg["base"], off, ln)
        _check(W.zlib_batch(seg["data"], off, ln), want, off, ln, "oracle against zlib")


# --- 2. fixed-record leg ------------------------------------------------------------------
@pytest.mark.parametrize("shift", W.FIXED_SHIFTS)
def test_fixed_two_slot_kernel_every_first_segment_length(ctx, shift):
    """crc32_fixed_kernel<FAST = false> (stride 4097: never the dword-aligned
    paths) over layout (e): every start offset mod 4096 for every length, with
    records that straddle 64-segment tiles (memset + atomicXor accumulation)
    and without (one plain store per record)."""
    lengths = W.fixed_lengths()
    n, stride = W.FIXED_N, W.FIXED_STRIDE
    data = O.gen_stream(0x5EED0052, 0, W.fixed_nbytes())
    d = _upload(ctx, data)
    out = _canary_out(ctx, n * len(lengths))
    try:
        for i, L in enumerate(lengths):
            ctx.crc32_fixed_device(d.ptr + shift, stride, L, n, out.ptr + 4 * n * i)
        ctx.sync()
        got = out.download(np.uint32).reshape(len(lengths), n)
    finally:
        d.free()
        out.free()
    start = (shift + np.arange(n, dtype=np.uint64) * np.uint64(stride))
    for i, L in enumerate(lengths):
        want = O.crc32_fixed(data[shift:], stride, L, n, threads=8)
        ln = np.full(n, L, dtype=np.uint32)
        if L == 131:
            _check(W.zlib_batch(data, start, ln), want, start, ln, "oracle against zlib")
        bad = np.nonzero(got[i] != want)[0]
        assert len(bad) == 0, (f"len {L}, shift {shift}: {len(bad)} of {n} differ; first (index, start % 4096, got, "
                               f"want): {[(int(j), int(start[j] % 4096), hex(got[i][j]), hex(want[j])) for j in bad[:8]]}")


# --- 3. lane x segment-count matrix -------------------------------------------------------
@pytest.fixture(scope="module")
def lanes(ctx):
    off, ln, meta = W.lane_matrix()
    data = O.gen_stream(0x5EED0053, 0, meta["nbytes"])
    d = _upload(ctx, data)
    want = O.crc32_batch(data, off, ln, threads=8)
    yield {"base": d.ptr, "data": data, "off": off, "ln": ln, "want": want}
    d.free()


@pytest.mark.parametrize("route", list(ROUTES))
def test_lane_matrix(ctx, lanes, route):
    """Routes walk and default.  Every (start lane, segment count): records
    ending inside their tile, exactly on lane 63, and carried over 1..4 tiles
    by the Horner step; empty records on lanes of their own."""
    _check_route(ctx, lanes["base"], lanes["off"], lanes["ln"], lanes["want"], route, "lane matrix")
    if route == "default":
        assert _declined(ctx, lanes["base"], lanes["off"], lanes["ln"])
        _check(W.zlib_batch(lanes["data"], lanes["off"], lanes["ln"]), lanes["want"], lanes["off"], lanes["ln"],
               "oracle against zlib")


# --- 4. window ring and n edges -------------------------------------------------------------
@pytest.fixture(scope="module")
def windows(ctx):
    """All batches of layout (c) over one payload, their descriptors back to
    back in one upload; batch i is records [at[i], at[i + 1])."""
    cases = W.window_cases()
    off = np.concatenate([c[1] for c in cases])
    ln = np.concatenate([c[2] for c in cases])
    at = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])])
    data = O.gen_stream(0x5EED0054, 0, W.WIN_BLOB)
    d, d_o, d_l = _upload(ctx, data), _upload(ctx, off), _upload(ctx, ln)
    want = O.crc32_batch(data, off, ln, threads=8)
    yield {"cases": cases, "at": at, "off": off, "ln": ln, "data": data, "want": want, "d": d, "d_o": d_o, "d_l": d_l}
    for b in (d, d_o, d_l):
        b.free()


@pytest.mark.parametrize("route", list(ROUTES))
def test_window_ring_and_batch_sizes(ctx, windows, route):
    """Route walk: every batch.  Route default: the batches stream_check
    declines as built (all but the packed ones with a non-empty first
    record).  One launch per batch, each into its own slice of `out`."""
    w = windows
    at, n = w["at"], len(w["off"])
    run = [i for i, (_, off, ln) in enumerate(w["cases"]) if route == "walk" or not W.stream_eligible(off, ln)]
    assert len(run) >= 64 * 11 + 6
    out = _canary_out(ctx, n)
    try:
        with _option(ctx, "crc_stream", ROUTES[route], 1):
            for i in run:
                a = int(at[i])
                ctx.crc32_device(w["d"].ptr, w["d_o"].ptr + 8 * a, w["d_l"].ptr + 4 * a, int(at[i + 1]) - a,
                                 out.ptr + 4 * a)
            ctx.sync()
        got = out.download(np.uint32)
    finally:
        out.free()
    ran = np.zeros(n, dtype=bool)
    for i in run:
        a, b = int(at[i]), int(at[i + 1])
        ran[a:b] = True
        _check(got[a:b], w["want"][a:b], w["off"][a:b], w["ln"][a:b], f"{w['cases'][i][0]} [{route}]")
    assert (got[~ran] == CANARY).all()      # no launch wrote outside its slice
    if route == "default":
        i = [c[0] for c in w["cases"]].index("p37_b129")
        a, b = int(at[i]), int(at[i + 1])
        assert _declined(ctx, w["d"].ptr, w["off"][a:b], w["ln"][a:b])
        _check(W.zlib_batch(w["data"], w["off"], w["ln"]), w["want"], w["off"], w["ln"], "oracle against zlib")


# --- 5. scale ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale_payload(ctx):
    data = O.gen_stream(0x5EED0055, 0, W.SCALE_BYTES)
    d = _upload(ctx, data)
    yield data, d
    d.free()


@pytest.mark.parametrize("n", W.SCALE_N)
def test_scale(ctx, scale_payload, n):
    """Route default.  n = 262,145: 1,025 superblocks, scan_phase2 with two
    per thread.  n = 4,194,309: 16,385 superblocks (17 per thread),
    walk_phase1's grid-stride loop, and crc32_verify_device over more records
    than crc32_compare_kernel has threads: the count and the first index of
    the mismatches when three expectations are wrong."""
    data, d = scale_payload
    off, ln = W.scale_batch(n)
    assert not W.stream_eligible(off, ln)
    want = O.crc32_batch(data, off, ln, threads=8)
    d_o, d_l, out = _upload(ctx, off), _upload(ctx, ln), _canary_out(ctx, n)
    d_e = None
    try:
        ctx.crc32_device(d.ptr, d_o.ptr, d_l.ptr, n, out.ptr)
        ctx.sync()
        _check(out.download(np.uint32), want, off, ln, f"scale n = {n} [default]")
        if n == W.SCALE_N[0]:
            out.upload(np.full(n, CANARY, dtype=np.uint32))
            with _option(ctx, "crc_stream", 2, 1):
                ctx.crc32_device(d.ptr, d_o.ptr, d_l.ptr, n, out.ptr)
                ctx.sync()
            assert (out.download(np.uint32) == CANARY).all()
            k = 20000
            _check(W.zlib_batch(data, off[:k], ln[:k]), want[:k], off[:k], ln[:k], "oracle against zlib")
        else:
            d_e = _upload(ctx, want)
            assert ctx.crc32_verify_device(d.ptr, d_o.ptr, d_l.ptr, d_e.ptr, n) == (0, 0, n)
            exp = want.copy()
            exp[[2_097_157, 3_000_000, n - 1]] ^= 0x80000001
            d_e.upload(exp)
            assert ctx.crc32_verify_device(d.ptr, d_o.ptr, d_l.ptr, d_e.ptr, n) == (1, 3, 2_097_157)
    finally:
        for b in (d_o, d_l, out, d_e):
            if b is not None:
                b.free()


# --- 6. stores stay inside `out` ------------------------------------------------------------------
GUARD = 64
GUARD_N = (1, 63, 64, 65, 4099)


def _guarded(ctx, n, launch):
    """Run launch(out_ptr) with out one dword behind a 256-byte boundary (the
    stream and ring kernels store 256-byte blocks with lane masks at both ends
    of a wave's range), GUARD canary dwords in front of that boundary and
    GUARD behind out's end.  Returns (the n outputs, the dwords around them)."""
    lead = GUARD + 1
    buf = ctx.alloc(4 * (lead + n + GUARD))
    try:
        assert buf.ptr % 256 == 0
        buf.upload(np.full(lead + n + GUARD, CANARY, dtype=np.uint32))
        launch(buf.ptr + 4 * lead)
        ctx.sync()
        got = buf.download(np.uint32)
    finally:
        buf.free()
    return got[lead:lead + n], np.concatenate([got[:lead], got[lead + n:]])


def _guard_desc(ctx, kind, n):
    rng = np.random.default_rng(60 + n)
    if kind == "walk":      # crc_stream 0, scattered records of 0..700 bytes
        ln = rng.integers(0, 701, n).astype(np.uint32)
        off = rng.integers(0, (1 << 20) - 700 - W.SLACK, n).astype(np.uint64)
        opt = 0
    else:                   # crc_stream 2, packed records of 64..400 bytes: the stream kernel takes them
        ln = rng.integers(64, 401, n).astype(np.uint32)
        off = np.uint64(3) + np.concatenate([[0], np.cumsum(ln[:-1].astype(np.uint64))]).astype(np.uint64)
        assert W.stream_eligible(off, ln)
        opt = 2
    return off, ln, opt


@pytest.mark.parametrize("kind", ["walk", "stream", "fixed_two_slot", "fixed_ring"])
def test_stores_stay_inside_out(ctx, kind):
    """Every kernel that stores CRCs, on an `out` at dword offset 1 with guard
    dwords on both sides: all n CRCs equal the oracle's and no guard dword
    changes.  walk: plain stores; stream and fixed_ring: masked 256-byte block
    stores; fixed_two_slot (len 297, stride 300: records straddle tiles): the
    memset of `out` and the atomicXor accumulation."""
    data = O.gen_stream(0x5EED0056, 0, 4 << 20)
    d = _upload(ctx, data)
    try:
        for n in GUARD_N:
            if kind in ("walk", "stream"):
                off, ln, opt = _guard_desc(ctx, kind, n)
                d_o, d_l = _upload(ctx, off), _upload(ctx, ln)
                try:
                    with _option(ctx, "crc_stream", opt, 1):
                        got, guard = _guarded(ctx, n, lambda o: ctx.crc32_device(d.ptr, d_o.ptr, d_l.ptr, n, o))
                finally:
                    d_o.free()
                    d_l.free()
                want = O.crc32_batch(data, off, ln, threads=8)
            else:
                shift, stride, L = (1, 300, 297) if kind == "fixed_two_slot" else (0, 256, 256)
                got, guard = _guarded(ctx, n, lambda o: ctx.crc32_fixed_device(d.ptr + shift, stride, L, n, o))
                want = O.crc32_fixed(data[shift:], stride, L, n, threads=8)
                off, ln = shift + np.arange(n, dtype=np.uint64) * np.uint64(stride), np.full(n, L, dtype=np.uint32)
            _check(got, want, off, ln, f"{kind}, n = {n}")
            touched = np.nonzero(guard != CANARY)[0]
            assert len(touched) == 0, (f"{kind}, n = {n}: guard dwords written at {touched[:8].tolist()} "
                                       f"(0..{GUARD}: in front of out, {GUARD + 1}..: behind it)")
    finally:
        d.free()


# --- 7. the comparison can fail ------------------------------------------------------------------
def test_comparison_reports_a_kernel_that_stores_nothing(ctx, seg):
    """crc_ablate 3 (lsmck.h: payload loads only, results invalid): the walking
    kernel stores nothing, every output keeps the canary, and the helper the
    tests above rely on reports every record."""
    p = seg["perm"]
    off, ln, want = seg["off"][p], seg["ln"][p], seg["want"][p]
    assert (want != CANARY).all()
    with _option(ctx, "crc_ablate", 3, 0):
        got = _crc(ctx, seg["base"], off, ln, 0)
    bad, msg = W.mismatches(got, want, off, ln)
    assert len(bad) == len(want) and bad[0] == 0 and msg.startswith(f"{len(want)} of {len(want)} CRCs differ")
    with pytest.raises(AssertionError):
        _check(got, want, off, ln)
    _check(_crc(ctx, seg["base"], off, ln, 0), want, off, ln, "after crc_ablate 0")
