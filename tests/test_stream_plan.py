"""The stream kernel's slice plan (csrc/lsmck_splan.h: the function stream_cut
runs on the device, built here as plain C++): for the slice counts the launcher
picks on a 256-CU device (W = 4096 waves) the cuts' byte fractions run from 0
to 1 without decreasing, the first W slices (one per wave, taken without a
ticket) are equal, every later slice is no larger than the one before, and the
count stays within the cut buffer's size.

Tolerance: the plan divides exact integer weights once, so each fraction is
within 2^-53 of p / total and a slice size (a difference of two) within 2^-52
of its exact value; sizes are compared with 2^-50 of slack."""
import numpy as np
import pytest

import splan_model

NCU = 256
W = 4096
EPS = 2.0 ** -50


@pytest.mark.parametrize("n", [64 * W, 64 * W + 64, 150 * W, 1 << 22, 1 << 26])
def test_plan_properties(n):
    lib = splan_model.load()
    assert lib.splan_waves(NCU) == W
    S = lib.splan_slices(NCU, n)
    assert W <= S <= lib.splan_slices_max(NCU)
    assert S <= max(W, n // 64)  # at least 64 records a slice once the slices outnumber the waves
    f = np.array([lib.splan_fraction(s, S, W) for s in range(S + 1)])
    assert f[0] == 0.0 and f[S] == 1.0
    size = np.diff(f)
    assert (size >= 0.0).all()
    assert np.abs(size[:W] - size[0]).max() <= EPS          # the untied first slices are equal
    assert (size[1:] <= size[:-1] + EPS).all()               # sizes never grow in ticket order
    assert size.min() > 0.0
    if S == W:
        assert np.abs(f - np.arange(S + 1) / S).max() <= EPS  # one slice per wave: equal shares


def test_plan_thresholds():
    lib = splan_model.load()
    n1 = splan_model.first_n_over_one_slice_per_wave(NCU)
    assert lib.splan_slices(NCU, n1 - 1) == W and lib.splan_slices(NCU, n1) == W + 1
    assert lib.splan_slices(NCU, 1) == W
    assert lib.splan_slices(NCU, 1 << 40) == lib.splan_slices_max(NCU)
    # the full plan spends most of its slices on the tail: the last slice is
    # well under an equal share of the slice count, the first well over it
    S = lib.splan_slices_max(NCU)
    first = lib.splan_fraction(1, S, W)
    last = 1.0 - lib.splan_fraction(S - 1, S, W)
    assert last <= 1.0 / S <= first
    # a slice costs its wave a restart: on the full workload (config 3: 2^26
    # records, 104,143,148,313 payload bytes) the smallest stays over 32 tiles of 8 KiB
    assert lib.splan_slices(NCU, 1 << 26) == S
    assert last * 104143148313 / 8192 >= 32.0
