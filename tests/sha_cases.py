"""Layouts and references for the SHA-256 edge tests (test_gpu_sha_edges.py).

The window paths of lsmck_sha256.hip branch on a message's length and on its
absolute start address: A & 3 picks the funnel shift, A & 127 the column of
the line-aligned path.  The layouts here therefore place messages at wanted
residues of the *absolute* address base + off (base: the device pointer the
payload is uploaded to), in increasing offset, not overlapping, with the
smallest gap that reaches the residue.

Nothing in this module needs a GPU: tests/test_sha_cases.py checks it.
"""
import hashlib

import numpy as np

LINE = 128

# the matrix of test_gpu_sha_edges.py section 1
DENSE_LENGTHS = range(0, 705)            # every start residue mod 128
DENSE_ALIGNS = tuple(range(LINE))
SPARSE_LENGTHS = range(705, 2241)        # up to 35 main blocks: nmain 0..35, npair 0..17
SPARSE_ALIGNS = (0, 1, 2, 3, 4, 60, 63, 64, 65, 124, 127)
SLACK = 4096  # bytes kept after the last message: no message lies against the end of its allocation


def matrix_pairs():
    """(length, alignment) of every message of the matrix, in layout order."""
    ln = np.concatenate([np.repeat(np.arange(DENSE_LENGTHS.start, DENSE_LENGTHS.stop), len(DENSE_ALIGNS)),
                         np.repeat(np.arange(SPARSE_LENGTHS.start, SPARSE_LENGTHS.stop), len(SPARSE_ALIGNS))])
    al = np.concatenate([np.tile(np.array(DENSE_ALIGNS), len(DENSE_LENGTHS)),
                         np.tile(np.array(SPARSE_ALIGNS), len(SPARSE_LENGTHS))])
    return ln.astype(np.uint32), al.astype(np.uint32)


def place(base_ptr, lengths, aligns, start=0):
    """Offsets (uint64) of messages of `lengths` laid out in order from
    `start`, message i at the first offset at or after the previous message's
    end with (base_ptr + off) % 128 == aligns[i].  Returns (off, total):
    total is the end of the last message."""
    off = np.empty(len(lengths), dtype=np.uint64)
    pos = int(start)
    base = int(base_ptr)
    for i, (l, a) in enumerate(zip(lengths.tolist(), aligns.tolist())):
        pos += (a - base - pos) % LINE
        off[i] = pos
        pos += l
    return off, pos


def packed(lengths, start=0):
    """Offsets of the messages back to back (gap 0) from `start`, and the end."""
    off = np.empty(len(lengths), dtype=np.uint64)
    ends = np.cumsum(lengths.astype(np.uint64)) + np.uint64(start)
    off[0:1] = start
    off[1:] = ends[:-1]
    return off, int(ends[-1]) if len(lengths) else int(start)


def alignments(base_ptr, off):
    """(base_ptr + off) % 128 per message."""
    return ((np.uint64(int(base_ptr) % LINE) + (off % np.uint64(LINE))) % np.uint64(LINE)).astype(np.uint32)


def main_pairs(base_ptr, off, ln):
    """npair of sha256_run (lsmck_sha256.hip) per message: the two-block load
    windows of the main loop.  With A = base + off, a40 = A & ~3 and end4 =
    (A + len + 3) & ~3, the main blocks are those whole 64-byte blocks whose
    68-byte dword window lies inside the message's dwords:

        nmain = min(len >> 6, (end4 - a40 - 68) / 64 + 1)   if len and end4 >= a40 + 68
                0                                           otherwise
        npair = nmain >> 1

    Only end4 - a40 enters, and that depends on A & 3 alone."""
    sh = (np.uint64(int(base_ptr) & 3) + (off & np.uint64(3))) & np.uint64(3)
    ln = ln.astype(np.int64)
    span = ((sh.astype(np.int64) + ln + 3) & ~np.int64(3))  # end4 - a40
    nsafe = np.where((ln > 0) & (span >= 68), (span - 68) // 64 + 1, 0)
    return (np.minimum(ln >> 6, nsafe) >> 1).astype(np.int64)


def hashlib_batch(data, off, ln):
    """SHA-256 of data[off[i] : off[i] + ln[i]) per message from the standard
    library, as an (n, 32) uint8 array."""
    mv = memoryview(np.ascontiguousarray(data, dtype=np.uint8)).cast("B")
    out = bytearray(32 * len(off))
    sha = hashlib.sha256
    for i, (o, l) in enumerate(zip(np.asarray(off).tolist(), np.asarray(ln).tolist())):
        out[32 * i:32 * i + 32] = sha(mv[o:o + l]).digest()
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(len(off), 32)


def mismatches(got, want, *columns, limit=8):
    """Indices where two digest arrays differ, and a readable list of the
    first few with the given per-message columns (name, array) beside them."""
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).any(axis=1))[0]
    head = [tuple([int(i)] + [int(c[i]) for _, c in columns]) for i in bad[:limit]]
    names = ", ".join(["index"] + [n for n, _ in columns])
    return bad, f"{len(bad)} of {len(want)} digests differ; first ({names}): {head}"


# --- section 2: long messages --------------------------------------------------
LONG_K = (16, 17, 20, 21, 22)
LONG_D = (-65, -9, -1, 0, 1, 55, 64, 127)
LONG_ALIGNS = (0, 1, 3, 127)


def long_batch(base_ptr, n_filler=2100, seed=5):
    """An ordered batch (n >= 2048): short filler of 0..900 bytes with the
    messages of 2^k + d bytes (k in LONG_K, d in LONG_D: keys with e = 10..16
    in ShaBucket) scattered among it, their start residues mod 128 cycling
    through LONG_ALIGNS; the filler's residues are random.  Returns (off, ln,
    total)."""
    rng = np.random.default_rng(seed)
    longs = np.array([(1 << k) + d for k in LONG_K for d in LONG_D], dtype=np.uint32)
    ln = rng.integers(0, 901, n_filler + len(longs)).astype(np.uint32)
    al = rng.integers(0, LINE, len(ln)).astype(np.uint32)
    at = np.sort(rng.choice(len(ln), size=len(longs), replace=False))
    ln[at] = longs[rng.permutation(len(longs))]
    al[at] = np.resize(np.array(LONG_ALIGNS, dtype=np.uint32), len(longs))
    off, total = place(base_ptr, ln, al)
    return off, ln, total


# --- section 6: slice edges of the whole-tree verify ------------------------------
SLICE_K = (0, 1, 2, 3)
SLICE_D = (-65, -64, -9, -8, -1, 0, 1, 55, 56, 63, 64)


def slice_sizes(slice_bytes):
    """Data file sizes k * slice + d around the slice edges (negative ones skipped)."""
    return [k * slice_bytes + d for k in SLICE_K for d in SLICE_D if k * slice_bytes + d >= 0]
