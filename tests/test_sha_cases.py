"""The fixtures of the SHA-256 edge tests (tests/sha_cases.py), without a GPU:
the matrix is complete, its layouts are sorted and disjoint and land on the
wanted residues of the absolute address for any base pointer, the window-count
model matches its definition, and the two references -- hashlib and the
oracle's C restatement -- agree on every message of the matrix."""
import numpy as np
import pytest

import sha_cases as S
from oracle import oracle as O

# device pointers as hipMalloc gives them, and ones that are not line aligned
BASES = [0, 0x7F2A00000000, 0x7F2A00000000 + 1, 0x7F2A00000000 + 67, 0x7F2A00000000 + 127, (1 << 47) + 4093]


def test_matrix_holds_every_pair_once():
    ln, al = S.matrix_pairs()
    pairs = list(zip(ln.tolist(), al.tolist()))
    want = {(l, a) for l in range(0, 705) for a in range(128)}
    want |= {(l, a) for l in range(705, 2241) for a in (0, 1, 2, 3, 4, 60, 63, 64, 65, 124, 127)}
    assert len(pairs) == 128 * 705 + 11 * 1536 == 107136
    assert len(set(pairs)) == len(pairs) and set(pairs) == want


@pytest.mark.parametrize("base", BASES)
def test_placed_layout_sorted_disjoint_aligned(base):
    ln, al = S.matrix_pairs()
    off, total = S.place(base, ln, al)
    o, l = off.astype(np.int64), ln.astype(np.int64)
    gap = o[1:] - (o[:-1] + l[:-1])
    assert (gap >= 0).all() and (gap < 128).all()  # sorted, disjoint, the smallest gap
    assert 0 <= o[0] < 128 and total == o[-1] + l[-1]
    assert [(base + x) % 128 for x in o.tolist()] == al.tolist()  # in Python integers
    assert np.array_equal(S.alignments(base, off), al)
    assert 58 << 20 < total < 66 << 20  # "about 60 MB"


def test_packed_layout():
    ln, _ = S.matrix_pairs()
    off, total = S.packed(ln, start=3)
    o, l = off.astype(np.int64), ln.astype(np.int64)
    assert o[0] == 3 and np.array_equal(o[1:], o[:-1] + l[:-1]) and total == o[-1] + l[-1]
    al = S.alignments(0x7F2A00000040, off)
    assert [(0x7F2A00000040 + x) % 128 for x in o[:5000].tolist()] == al[:5000].tolist()
    assert len(set(al.tolist())) == 128  # every residue falls out


def _main_pairs_by_definition(A, n):
    """Count the blocks b with 64 (b + 1) <= n whose dword window [a40 + 64 b,
    a40 + 64 b + 68) ends at or before end4, one by one."""
    a40, end4 = A & ~3, (A + n + 3) & ~3
    nmain = 0
    while n and 64 * (nmain + 1) <= n and a40 + 64 * nmain + 68 <= end4:
        nmain += 1
    return nmain >> 1


@pytest.mark.parametrize("base", BASES[:4])
def test_main_pairs_model(base):
    ln, al = S.matrix_pairs()
    off, _ = S.place(base, ln, al)
    got = S.main_pairs(base, off, ln)
    idx = np.r_[0:len(ln):37, len(ln) - 2000:len(ln)]
    assert [_main_pairs_by_definition(base + int(off[i]), int(ln[i])) for i in idx] == got[idx].tolist()
    assert set(got.tolist()) == set(range(18))  # npair 0..17: every p % 3 tail of the line loop, up to 5 rounds
    # 256 bytes: dword aligned, the fourth block's 68-byte window ends past the message (one pair and
    # two blocks for the loader); otherwise its funnel dword is the message's last, partial one (two pairs)
    k2 = np.nonzero(ln == 256)[0]
    assert {((base + int(o)) & 3 == 0, int(p)) for o, p in zip(off[k2], got[k2])} == {(True, 1), (False, 2)}


def test_long_batch():
    base = 0x7F2A00000000 + 64
    off, ln, total = S.long_batch(base)
    assert len(ln) >= 2048
    longs = sorted((1 << k) + d for k in S.LONG_K for d in S.LONG_D)
    at = np.nonzero(ln > 900)[0]
    assert sorted(ln[at].tolist()) == longs and ln.max() == (4 << 20) + 127
    assert S.alignments(base, off)[at].tolist() == (list(S.LONG_ALIGNS) * len(longs))[:len(longs)]
    o, l = off.astype(np.int64), ln.astype(np.int64)
    assert (o[1:] >= o[:-1] + l[:-1]).all() and total == o[-1] + l[-1]
    # ShaBucket's log-spaced keys: e = floor(log2(blocks)) from 10 to 16
    nb = (l[at] + 72) >> 6
    assert {int(b).bit_length() - 1 for b in nb} >= {10, 11, 14, 15, 16}


def test_slice_sizes():
    for s in (64, 4096):
        z = S.slice_sizes(s)
        assert min(z) == 0 and max(z) == 3 * s + 64 and all(x >= 0 for x in z)
        assert {2 * s, 3 * s, s - 1, s + 1, 2 * s - 9, 3 * s + 55} <= set(z)


def test_hashlib_and_oracle_agree_on_the_matrix():
    ln, al = S.matrix_pairs()
    off, total = S.place(0x7F2A00000000, ln, al)
    data = O.gen_stream(0x5EED0A11, 0, total + 8)
    a, b = S.hashlib_batch(data, off, ln), O.sha256_batch(data, off, ln, threads=8)
    bad, msg = S.mismatches(a, b, ("length", ln), ("alignment", al))
    assert not len(bad), msg
    # no two messages of 8 bytes or more share a digest: the data never repeats
    assert len({r.tobytes() for r in a[ln >= 8]}) == int((ln >= 8).sum())
