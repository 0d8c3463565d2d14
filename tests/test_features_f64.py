"""Upsampling by 2 / 4 / 8 and noise synthesis against tests/features_f64.py, on the CPU: the host's kernel table, the
oracle's Upsample and AddNoise (through jxlo_upsample_kat / jxlo_noise_kat, on caller planes: no stream), the reading's
generator against the reference's golden values, and the proof that the listed cases tell the named misreadings apart.
tests/test_gpu_features_f64.py holds the HIP kernels to the same reading on the same cases."""
import ctypes

import numpy as np
import pytest

import features_f64 as F
from test_oracle import XORSHIFT_12345


# ---- the oracle on caller planes
def _olib():
    import jxlo
    L = jxlo.lib()
    L.jxlo_upsample_kat.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.jxlo_upsample_kat.restype = None
    L.jxlo_noise_kat.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                 ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    L.jxlo_noise_kat.restype = None
    return L


def oracle_upsample(plane, n, weights, oxs, oys):
    L = _olib()
    plane = np.ascontiguousarray(plane, np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    out = np.empty((oys, oxs), np.float32)
    L.jxlo_upsample_kat(plane.ctypes.data, plane.shape[1], plane.shape[0], n, None if w is None else w.ctypes.data, oxs, oys, out.ctypes.data, None)
    return out


def oracle_noise(xyb, seed0, seed1, lut, ytox, ytob):
    L = _olib()
    out = np.ascontiguousarray(xyb, np.float32).copy()
    raw = np.empty_like(out)
    lut = np.ascontiguousarray(lut, np.float32)
    L.jxlo_noise_kat(out.ctypes.data, out.shape[2], out.shape[1], seed0, seed1, lut.ctypes.data, ytox, ytob, raw.ctypes.data)
    return out, raw


def upsample_cases():
    """(xs, ys, n, weights or None, content, (oxs, oys)) of every listed case."""
    for xs, ys in F.UPSAMPLE_SIZES:
        for n in (2, 4, 8):
            for weights in (None, "coded"):
                for content in ("noise", "step", "constant"):
                    for size in F.out_sizes(xs, ys, n):
                        yield xs, ys, n, weights, content, size


def noise_cases():
    """(xs, ys, seeds, lut) of every listed case. Each size runs one seed pair with each table, and the seed pairs rotate
    over the sizes; the largest size, where the generator costs the most, runs once per table."""
    for i, (xs, ys) in enumerate(F.NOISE_SIZES):
        for j, lut in enumerate((F.LUT_RAMP, F.LUT_WITH_ZERO)):
            yield xs, ys, F.NOISE_SEEDS[(i + j) % 3], lut
    for seeds in F.NOISE_SEEDS:  # every seed pair on a size with two squares and on the smallest
        yield 257, 3, seeds, F.LUT_RAMP
        yield 1, 1, seeds, F.LUT_WITH_ZERO


YTOX, YTOB = 0.25, 0.75  # a coded base correlation (the default 0, 1 would hide X's and B's products)


# ---- the host's kernel table
def stream_coded_weights(seed):
    """What libjxl_amd.set_custom_upsampling(7, seed) makes the encoder write (its recipe, restated: the default weights
    times 0.75 + 0.5 r, r from a 32-bit linear congruential generator, rounded to binary16), for n = 2, 4, 8."""
    st = (seed * 2654435761 + 12345) & 0xFFFFFFFF
    out = {}
    for n in (2, 4, 8):
        w = []
        for d in F.default_weights(n):
            st = (st * 1664525 + 1013904223) & 0xFFFFFFFF
            r = np.float32(0.75) + np.float32((st >> 8) * 0.5 / 16777216.0)
            v = np.float32(d * r)
            bits = (int(v.view(np.uint32)) + 0x1000) & ~0x1FFF & 0xFFFFFFFF
            v = np.uint32(bits).view(np.float32)
            w.append(np.float32(0) if abs(v) < 6.2e-5 else v)
        out[n] = np.asarray(w, np.float32)
    return out


@pytest.mark.parametrize("seed", [None, 3, 11])
def test_host_kernel_table_is_the_reading(built, seed):
    """jxlamd_upsampling_kernels == upsampling_kernels, exactly, for the default weights and two coded sets."""
    J = built
    img = J.synth_image(24, 16, seed=2)
    if seed is None:
        data, weights = J.encode_rgb8(img, upsampling=2), {2: None, 4: None, 8: None}
    else:
        J.set_custom_upsampling(7, seed)
        try:
            data = J.encode_rgb8(img, upsampling=2)
        finally:
            J.set_custom_upsampling(0)
        weights = stream_coded_weights(seed)
        assert not np.array_equal(weights[4], F.default_weights(4))
    f = J.Frame(data)
    try:
        for n in (2, 4, 8):
            assert np.array_equal(f.upsampling_kernels(n), F.upsampling_kernels(n, weights[n])), n
    finally:
        f.close()


def test_kernels_are_symmetric_and_sum_to_one():
    """What the default weights must satisfy whoever reads them: every kernel sums to 1 and the table has the four mirror
    symmetries (a transposed or unflipped reading of the triangle breaks one of the two)."""
    for n in (2, 4, 8):
        k = F.upsampling_kernels(n).astype(np.float64)
        assert np.abs(k.sum(axis=(2, 3)) - 1).max() < 2e-6
        assert np.array_equal(k, k[::-1, :, ::-1, :]) and np.array_equal(k, k[:, ::-1, :, ::-1])
        assert np.array_equal(k, k.transpose(1, 0, 3, 2))


# ---- the oracle against the reading
def test_reading_reproduces_the_generator_golden_values():
    got = F.xorshift_single_seed(12345, len(XORSHIFT_12345))
    assert [[int(v) for v in row] for row in got] == XORSHIFT_12345


def test_oracle_sits_within_the_bars(built):
    """The oracle within the bar of the reading on every listed case; raw noise bit for bit. Prints the oracle's largest
    distance in units of the DERIVED bars: the figures features_f64.ORACLE_*_DISTANCE record (measured: upsampling 0.0821,
    noise 0.2058), which must not be exceeded, since the bars in use are sized by them."""
    worst_up = 0.0
    for xs, ys, n, weights, content, (oxs, oys) in upsample_cases():
        w = None if weights is None else F.coded_weights(n)
        plane = F.upsample_plane_case(xs, ys, content)
        want, mag = F.upsample(plane, n, F.upsampling_kernels(n, w), oxs, oys)
        got = oracle_upsample(plane, n, w, oxs, oys).astype(np.float64)
        derived = F.upsample_bar(want, mag) / F.UPSAMPLE_BAR_SCALE
        worst_up = max(worst_up, float((np.abs(got - want) / derived).max()))
        if content == "constant":
            assert (got == plane[0, 0]).all()
    worst_noise = 0.0
    for xs, ys, seeds, lut in noise_cases():
        xyb = F.noise_planes_case(xs, ys)
        want, bar, bits = F.noise(xyb, seeds[0], seeds[1], lut, YTOX, YTOB)
        got, raw = oracle_noise(xyb, seeds[0], seeds[1], lut, YTOX, YTOB)
        assert np.array_equal(raw.view(np.uint32), bits), (xs, ys, seeds)
        worst_noise = max(worst_noise, float((np.abs(got - want) / (bar / F.NOISE_BAR_SCALE)).max()))
    print("oracle's largest distance / derived bar: upsampling %.4f, noise %.4f" % (worst_up, worst_noise))
    assert worst_up <= F.ORACLE_UPSAMPLE_DISTANCE and worst_noise <= F.ORACLE_NOISE_DISTANCE
    # (so the oracle is within the bars in use: they are the derived ones, or 4 times the recorded distance)
    assert F.ORACLE_UPSAMPLE_DISTANCE < F.UPSAMPLE_BAR_SCALE and F.ORACLE_NOISE_DISTANCE < F.NOISE_BAR_SCALE


# ---- the cases tell the misreadings apart
@pytest.mark.parametrize("name", F.UPSAMPLE_MISREADINGS)
def test_upsampling_misreading_shows(name):
    worst = 0.0
    for xs, ys, n, weights, content, (oxs, oys) in upsample_cases():
        if content == "constant" or worst > 10:
            continue
        w = None if weights is None else F.coded_weights(n)
        plane = F.upsample_plane_case(xs, ys, content)
        want, mag = F.upsample(plane, n, F.upsampling_kernels(n, w), oxs, oys)
        table = F.upsampling_kernels(n, w, misread=name)
        wrong, _ = F.upsample(plane, n, table, oxs, oys, misread=name)
        worst = max(worst, float((np.abs(wrong - want) / F.upsample_bar(want, mag)).max()))
    assert worst > 10, worst


@pytest.mark.parametrize("name", F.NOISE_MISREADINGS)
def test_noise_misreading_shows(name):
    worst = 0.0
    for xs, ys, seeds, lut in noise_cases():
        if worst > 10 or xs * ys > 4000:  # (the large case is not needed to tell any of them apart)
            continue
        xyb = F.noise_planes_case(xs, ys)
        want, bar, _ = F.noise(xyb, seeds[0], seeds[1], lut, YTOX, YTOB)
        wrong, _, _ = F.noise(xyb, seeds[0], seeds[1], lut, YTOX, YTOB, misread=name)
        worst = max(worst, float((np.abs(wrong - want) / bar).max()))
    assert worst > 10, worst


def test_order_misreading_shows():
    """Noise before the upsampling instead of behind it, on frame planes 130 x 7 twice upsampled."""
    xs, ys, n = 130, 7, 2
    xyb = F.noise_planes_case(xs, ys)
    k = F.upsampling_kernels(n)
    want, bar = F.features(xyb, n, k, xs * n, ys * n, 0, 0, F.LUT_RAMP, YTOX, YTOB)
    wrong, _ = F.features(xyb, n, k, xs * n, ys * n, 0, 0, F.LUT_RAMP, YTOX, YTOB, misread="noise_before_upsampling")
    assert (np.abs(wrong - want) / bar).max() > 10


# ---- coverage of the clamp and of the strength table's ends
def test_the_clamp_bites_on_the_step_planes():
    """At least 1 % of the reading's outputs on the step-edge planes differ from the unclamped sum (measured with
    STEP_AMPLITUDE 1.0 over Gaussian noise of sigma 0.05: 18.3 %), on both sides of the window's range."""
    total = clamped = low = high = 0
    for xs, ys, n, weights, content, (oxs, oys) in upsample_cases():
        if content != "step":
            continue
        w = None if weights is None else F.coded_weights(n)
        plane = F.upsample_plane_case(xs, ys, content)
        k = F.upsampling_kernels(n, w)
        with_clamp, _ = F.upsample(plane, n, k, oxs, oys)
        without, _ = F.upsample(plane, n, k, oxs, oys, misread="no_clamp")
        total += with_clamp.size
        clamped += int((with_clamp != without).sum())
        low += int((with_clamp > without).sum())
        high += int((with_clamp < without).sum())
    print("clamped share of the step planes: %.4f" % (clamped / total))
    assert clamped >= 0.01 * total and low > 0 and high > 0


def test_strength_inputs_span_the_table_and_both_ends():
    for xs, ys in F.NOISE_SIZES:
        if xs * ys < 30:
            continue
        x, y, _ = F.noise_planes_case(xs, ys).astype(np.float64)
        for v in ((y - x) * 3.0, (y + x) * 3.0):
            assert (v < 0).any() and ((v >= 0) & (v < 7)).any() and (v >= 7).any(), (xs, ys)
    # the table itself at its ends and between two points
    lut = np.arange(8.0) / 10
    assert np.allclose(F.noise_strength(lut, np.array([-1.0, 0.0, 0.25, 7 / 6, 5.0])), [0.0, 0.0, 0.15, 0.7, 0.7])
