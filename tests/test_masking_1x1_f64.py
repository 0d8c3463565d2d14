"""The reference's per-pixel masking (mask1x1) as the CPU stream writer states it (jxlenc_cpu_masking_1x1, the double of
the device's jxlhip_enc_masking_1x1) against the float64 reading of tests/masking_1x1_f64.py, which shares no code with
it. This is where RTOL_MEASURED and RTOL_DARK_MEASURED of that file were measured for the CPU double: run with -s, every
test prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import adaptive_quant_f64 as A
import masking_1x1_f64 as M


@functools.lru_cache(maxsize=None)
def planes(kind, size):
    p = A.crafted(kind, size[0], size[1])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reading(kind, size, wrong=None):
    m = M.masking_1x1(planes(kind, size), wrong)
    m.setflags(write=False)
    return m


def check_entry(J, ctx, kind):
    """One plane kind over every size: mask1x1 of the stand-alone entry (the device's on `ctx`, the CPU double's without)
    within the kind's tolerance of the reading, relative, at every pixel. Returns the largest deviation."""
    worst, bad = 0.0, []
    for size in M.SIZES:
        want = reading(kind, size)
        got = J.masking_1x1(planes(kind, size), ctx=ctx)
        assert got.shape == want.shape == (size[1], size[0]) and got.dtype == np.float32
        dev = float(np.max(np.abs(got - want) / np.abs(want)))
        worst = max(worst, dev)
        if not dev <= M.rtol(kind):
            bad.append((size, dev))
    print("%s: largest relative deviation %.3e (tolerance %.3e)" % (kind, worst, M.rtol(kind)))
    assert not bad, bad
    return worst


def check_misreading(J, ctx, wrong):
    """The product lies further than the tolerance from the misreading `wrong` on some plane of every size class that
    can show it (all of them: a misreading of the border shows at every size, one of the pixel rule too)."""
    for size in M.SIZES:
        margin = 0.0
        for kind in M.KINDS:
            got = J.masking_1x1(planes(kind, size), ctx=ctx)
            dev = float(np.max(np.abs(got - reading(kind, size, wrong)) / np.abs(reading(kind, size))))
            margin = max(margin, dev / M.rtol(kind))
        print("%s at %dx%d: %.1f tolerances away" % (wrong, size[0], size[1], margin))
        assert margin > 4.0, (wrong, size, margin)


@pytest.mark.parametrize("kind", M.KINDS)
def test_cpu_entry_matches_float64_reading(built, kind):
    check_entry(built, None, kind)


@pytest.mark.parametrize("wrong", M.MISREADINGS)
def test_each_misreading_bites(built, wrong):
    check_misreading(built, None, wrong)


def test_reading_is_a_weighted_mean_and_the_planes_reach_both_classes():
    """Judged by the reading alone: the 25 weights sum to 1, so a flat plane gives 1 / 0.01 everywhere; the corner weight D
    and the knight's-move weight L differ (or their order could not matter); the dark kind drives Y + 0.019 below zero and
    the others do not; the sizes put pixels within two of both edges of each axis and, at 200x136, further than that."""
    k = M.blur_kernel()
    assert abs(k.sum() - 1.0) < 1e-7 and np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and k[0, 0] != k[0, 1]
    assert np.allclose(reading("flat", (72, 40)), 100.0, rtol=1e-12)
    for kind in M.KINDS:
        dark = bool((planes(kind, (200, 136))[1] + np.float32(0.019) < 0).any())
        assert dark == (kind in M.DARK_KINDS), kind
    assert min(M.SIZES) == (8, 8) and max(M.SIZES) == (200, 136)


def test_entry_rejects_bad_arguments(built):
    J = built
    with pytest.raises(J.JxlAmdError):
        J.masking_1x1(np.zeros((3, 12, 8), np.float32))
    with pytest.raises(J.JxlAmdError):
        J.masking_1x1(np.zeros((3, 8, 20), np.float32))
    with pytest.raises(ValueError):
        J.masking_1x1(np.zeros((8, 8), np.float32))


def test_only_the_y_plane_is_read(built):
    J = built
    p = planes("noise", (72, 40)).copy()
    want = J.masking_1x1(p)
    p[0] += 0.25
    p[2] = 0.0
    assert np.array_equal(J.masking_1x1(p), want)
