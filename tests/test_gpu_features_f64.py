"""The HIP upsampling and noise kernels (-m gpu) against tests/features_f64.py, the reading of the reference's text that
shares no code with the kernels, the host library or the oracle: k_upsample_plane through jxlhip_upsample_plane and
k_noise_random / k_noise_add through jxlhip_debug_noise on the synthetic cases of test_features_f64.py (sizes below a tile,
where the mirror bounces more than once; ragged last columns; every generator lane; squares of 256, 256 and 1 .. 17),
k_upsample_color on streams, from the device's own filtered planes, and the order upsampling -> noise on one stream.
The bars are features_f64's (derived there, checked against the oracle's distance on the CPU); the colour stage behind
k_upsample_color is held to the bar test_gpu_color_encoding.py holds k_color_out to for an sRGB target (2e-4)."""
import ctypes

import numpy as np
import pytest

import color_encoding_f64 as C
import features_f64 as F
import test_features_f64 as S

pytestmark = pytest.mark.gpu

INVALID = 1  # JXLHIP_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def ctx(built):
    c = built.HipContext()
    yield c
    c.close()


# ---- k_upsample_plane
def test_upsample_plane_on_synthetic_planes(ctx):
    worst, bad = 0.0, []
    for xs, ys, n, weights, content, (oxs, oys) in S.upsample_cases():
        w = None if weights is None else F.coded_weights(n)
        plane = F.upsample_plane_case(xs, ys, content)
        k = F.upsampling_kernels(n, w)
        want, mag = F.upsample(plane, n, k, oxs, oys)
        got = ctx.upsample_plane(plane, n, k, oxs, oys)
        assert got.shape == want.shape
        d = float((np.abs(got.astype(np.float64) - want) / F.upsample_bar(want, mag)).max())
        worst = max(worst, d)
        if d > 1 or (content == "constant" and not (got == plane[0, 0]).all()):
            bad.append((xs, ys, n, weights, content, oxs, oys, d))
    print("k_upsample_plane: largest distance / bar %.3f" % worst)
    assert not bad, bad[:8]


def test_upsample_plane_as_the_alpha_plane(built, ctx):
    """as_alpha = 1: the result stays on the device as the alpha plane of the uploaded frame (129 x 17: the ragged size of a
    65 x 9 plane twice upsampled) and comes back through jxlhip_download_alpha."""
    J = built
    xs, ys, n, oxs, oys = 65, 9, 2, 129, 17
    f = J.Frame(J.encode_rgb8(J.synth_image(oxs, oys, seed=4)))
    try:
        ctx.upload(f)
        plane = F.upsample_plane_case(xs, ys, "step")
        k = F.upsampling_kernels(n)
        assert ctx.upsample_plane(plane, n, k, oxs, oys, as_alpha=True) is None
        got = ctx.download_alpha(oxs, oys).astype(np.float64)
        assert J.lib().jxlhip_set_alpha(ctx._h, None, 0, 0) == 0  # (the shared context goes on without alpha)
    finally:
        f.close()
    want, mag = F.upsample(plane, n, k, oxs, oys)
    assert (np.abs(got - want) <= F.upsample_bar(want, mag)).all()


def test_upsample_plane_refuses_what_it_cannot_index(built, ctx):
    L = built.lib()
    L.jxlhip_upsample_plane.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    plane, k, out = np.zeros((3, 5), np.float32), np.zeros(64 * 25, np.float32), np.zeros(64 * 64, np.float32)
    p, kp, op = plane.ctypes.data, k.ctypes.data, out.ctypes.data
    for args in ((p, 5, 3, 3, kp, 15, 9, 0, op),    # not a factor
                 (p, 5, 3, 2, kp, 11, 6, 0, op),    # the output needs more columns than the plane has
                 (p, 5, 3, 2, kp, 10, 4, 0, op),    # ... fewer rows than the plane has
                 (p, 0, 3, 2, kp, 10, 6, 0, op), (None, 5, 3, 2, kp, 10, 6, 0, op), (p, 5, 3, 2, None, 10, 6, 0, op)):
        assert L.jxlhip_upsample_plane(ctx._h, *args) == INVALID, args[1:4]


# ---- k_upsample_color
def _decode(J, data, keep, out_format=None):
    """One frame through the stages: (pixels, xyb_filtered cropped to the frame, xyb_upsampled cropped to the image or None, route)."""
    f = J.Frame(data)
    c = J.HipContext()
    try:
        c.set_option("keep_filtered", 1)
        c.set_option("keep_upsampled", 1 if keep else 0)
        if out_format is not None:
            c.set_output_format(*out_format)
        c.upload(f)
        c.run_all()
        c.sync()
        r, flags = c.errors()
        assert r == 0 and not any(flags)
        fi = c.frame_info
        filt = c.download("xyb_filtered")[:, :fi["ysize"], :fi["xsize"]].copy()
        if keep:
            up = c.download("xyb_upsampled")[:, :, :fi["out_xsize"]].copy()
        else:
            up = None
            assert lib_download_refused(J, c, "xyb_upsampled")
        return c.pixels(), filt, up, c.pixel_route()
    finally:
        c.close()
        f.close()


def lib_download_refused(J, c, name):
    need = ctypes.c_size_t()
    return J.lib().jxlhip_download(c._h, name.encode(), None, 0, ctypes.byref(need)) == INVALID


def _srgb_of(xyb):
    """XYB planes [3][ys][xs] -> sRGB-encoded [ys][xs][3], the float64 reading of the colour stage for an sRGB image."""
    _, ys, xs = xyb.shape
    lin = C.output_matrix(C.SRGB, C.D65) @ C.xyb_to_mixed(xyb.reshape(3, -1))
    return C.render(lin, "srgb", 255.0, "srgb").T.reshape(ys, xs, 3)


@pytest.mark.parametrize("size,n", [((141, 67), 2), ((141, 67), 4), ((141, 67), 8), ((8, 8), 8)])
def test_upsample_color_from_the_device_s_own_filtered_planes(built, size, n):
    J = built
    data = J.encode_rgb8(J.synth_image(size[0], size[1], seed=30 + n), upsampling=n)
    k = F.upsampling_kernels(n)
    # with keep_upsampled: the planes the kernel writes
    _, filt, up, route_kept = _decode(J, data, True)
    assert filt.shape[1:] == (-(-size[1] // n), -(-size[0] // n)) and up.shape == (3, size[1], size[0])
    want, bar = [], []
    for c in range(3):
        w, mag = F.upsample(filt[c], n, k, size[0], size[1])
        want.append(w)
        bar.append(F.upsample_bar(w, mag))
    want, bar = np.stack(want), np.stack(bar)
    d = np.abs(up.astype(np.float64) - want) / bar
    print("k_upsample_color planes: largest distance / bar %.3f" % d.max())
    assert (d <= 1).all()
    # the default route, where the kernel makes the pixels itself: f32, then 8 bits
    exp = _srgb_of(want)
    f32, filt2, _, route = _decode(J, data, False, (0, 3))
    assert np.array_equal(filt2, filt) and route == route_kept == 0
    print("k_upsample_color f32 sRGB: largest distance %.3g" % np.abs(f32 - exp).max())
    assert np.abs(f32.astype(np.float64) - exp).max() <= 2e-4
    u8, _, _, route = _decode(J, data, False)
    assert route == 0 and u8.dtype == np.uint8
    # (dither below half a level + rounding half a level + the f32 bar)
    assert np.abs(u8.astype(np.float64) - np.clip(exp, 0, 1) * 255).max() <= 1.0 + 255 * 2e-4


# ---- noise
def test_noise_kernels_on_synthetic_planes(ctx):
    worst, bad = 0.0, []
    for xs, ys, seeds, lut in S.noise_cases():
        xyb = F.noise_planes_case(xs, ys)
        want, bar, bits = F.noise(xyb, seeds[0], seeds[1], lut, S.YTOX, S.YTOB)
        got, raw = ctx.debug_noise(xyb, seeds[0], seeds[1], lut, S.YTOX, S.YTOB)
        assert np.array_equal(raw.view(np.uint32), bits), (xs, ys, seeds)
        d = float((np.abs(got.astype(np.float64) - want) / bar).max())
        worst = max(worst, d)
        if d > 1:
            bad.append((xs, ys, seeds, d))
    print("k_noise_add: largest distance / bar %.3f" % worst)
    assert not bad, bad


def test_noise_band_leaves_the_other_rows_alone(ctx):
    xs, ys = 33, 5
    xyb = F.noise_planes_case(xs, ys)
    whole, _ = ctx.debug_noise(xyb, 3, 7, F.LUT_RAMP, S.YTOX, S.YTOB)
    band, raw = ctx.debug_noise(xyb, 3, 7, F.LUT_RAMP, S.YTOX, S.YTOB, band=(1, 3), want_raw=False)
    assert raw is None
    assert np.array_equal(band[:, 1:3].view(np.uint32), whole[:, 1:3].view(np.uint32))
    for rows in (slice(0, 1), slice(3, 5)):
        assert np.array_equal(band[:, rows].view(np.uint32), xyb[:, rows].view(np.uint32))
    assert not np.array_equal(whole[:, 0], xyb[:, 0])


def test_noise_entry_refuses_bad_arguments(built, ctx):
    L = built.lib()
    L.jxlhip_debug_noise.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_float, ctypes.c_float,
                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    xyb, out = np.zeros((3, 4, 6), np.float32), np.zeros((3, 4, 6), np.float32)
    lut, nan_lut = np.zeros(8, np.float32), np.full(8, np.nan, np.float32)
    p, o, t, nt = xyb.ctypes.data, out.ctypes.data, lut.ctypes.data, nan_lut.ctypes.data
    for args in ((p, 0, 4, 0, 0, t, 0.0, 1.0, 0, 4, None, o), (p, 6, 0, 0, 0, t, 0.0, 1.0, 0, 4, None, o),  # no samples
                 (p, 6, 4, 0, 0, t, 0.0, 1.0, 2, 2, None, o), (p, 6, 4, 0, 0, t, 0.0, 1.0, 3, 2, None, o),  # no rows
                 (p, 6, 4, 0, 0, t, 0.0, 1.0, 0, 5, None, o),                                               # rows past the image
                 (p, 1 << 15, 1 << 15, 0, 0, t, 0.0, 1.0, 0, 4, None, o),                                  # more than 2^24 samples
                 (p, 6, 4, 0, 0, nt, 0.0, 1.0, 0, 4, None, o), (p, 6, 4, 0, 0, t, float("inf"), 1.0, 0, 4, None, o),
                 (None, 6, 4, 0, 0, t, 0.0, 1.0, 0, 4, None, o), (p, 6, 4, 0, 0, None, 0.0, 1.0, 0, 4, None, o),
                 (p, 6, 4, 0, 0, t, 0.0, 1.0, 0, 4, None, None)):
        assert L.jxlhip_debug_noise(ctx._h, *args) == INVALID, args[1:3] + args[8:10]
    assert L.jxlhip_debug_noise(None, p, 6, 4, 0, 0, t, 0.0, 1.0, 0, 4, None, o) == INVALID
    assert not out.any()


# ---- order and resolution
def test_noise_follows_the_upsampling_at_the_image_s_resolution(built):
    """515 x 259, twice upsampled, with noise: squares 256, 256 and 3 wide, 256 and 3 high, seeded by their origin in the
    IMAGE. The stream's table is the generator's documented one (point i = min(1023, noise + 40 i) / 1024), its base
    correlation the default (0, 1), its frame indices (0, 0)."""
    J = built
    xs, ys, n, strength = 515, 259, 2, 120
    data = J.encode_rgb8(J.synth_image(xs, ys, seed=77), upsampling=n, noise=strength)
    lut = np.minimum(1023, strength + 40 * np.arange(8)).astype(np.float32) / np.float32(1024)
    _, filt, up, route = _decode(J, data, True)
    assert route == 0 and up.shape == (3, ys, xs) and filt.shape == (3, 130, 258)
    want, bar = F.features(filt, n, F.upsampling_kernels(n), xs, ys, 0, 0, lut, 0.0, 1.0)
    d = np.abs(up.astype(np.float64) - want) / bar
    print("upsampling then noise: largest distance / bar %.3f" % d.max())
    assert (d <= 1).all()
    plain = np.stack([F.upsample(filt[c], n, F.upsampling_kernels(n), xs, ys)[0] for c in range(3)])
    assert np.abs(want - plain).max() > 1e-3  # (the noise is there)
