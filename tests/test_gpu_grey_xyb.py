"""Grey XYB images decoded on the GPU through the JxlDecoder API. The yardstick is the untagged twin, as in
tests/test_gpu_color_encoding.py: for a body B the stream S (untagged, colour) and the stream T (tagged Gray) share every
byte behind the header, S's linear-sRGB f32 decode is the oracle-pinned path, and T's pixels must be a float64 reading
(luminance 0.2126 R + 0.7152 G + 0.0722 B of S's linear pixels, then tests/color_encoding_f64.py) of S's pixels, never of
anything T's own decode produced. The bodies are coloured, so a writer that merely picked a channel fails. Every
comparison covers all samples."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import color_api as A
import color_encoding_f64 as C

pytestmark = pytest.mark.gpu

W, H = 600, 520  # several 256 x 256 groups, partial groups at both edges
LUMA = np.array([0.2126, 0.7152, 0.0722])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grey_ce(tf=13, gamma=0.0):
    ce = A.srgb_encoding()
    ce.color_space, ce.transfer_function, ce.gamma = 1, tf, gamma
    return ce


def _grey(J, encode, **kw):
    """encode() with colour space Gray (D65) declared on the header: the same XYB body as without it."""
    J.set_xyb_color_encoding(**dict(dict(white_point=1, transfer_function=13, gray=True), **kw))
    try:
        return encode()
    finally:
        J.set_xyb_color_encoding(None)


def _decode(L, data, shape, data_type=0, out=None):
    """[ys, xs, nc] through the API; out = a CE for JxlDecoderSetOutputColorProfile (None: the default)."""
    d = A.Decoder(L, data)
    try:
        assert d.status == 0x100, (d.status, L.jxlamd_last_error())
        if out is not None:
            assert d.set_output(out) == 0
        return d.decode(data_type, shape[2]).reshape(shape)
    finally:
        d.close()


def _luma_of_twin(L, S, shape=(H, W)):
    """The reading's input: the luminance of S's linear sRGB f32 pixels, in float64."""
    lin = _decode(L, S, shape + (3,), 0, A.srgb_encoding(linear=True)).astype(np.float64)
    return lin @ LUMA


def _render(y, tf, intensity=255.0, inv_gamma=None):
    """The grey image's own encoding of linear luminance y (any shape): the reading on three equal channels."""
    flat = np.broadcast_to(y.reshape(1, -1), (3, y.size))
    return C.render(flat, tf, intensity, tf, inv_gamma=inv_gamma)[0].reshape(y.shape)


@pytest.fixture(scope="module")
def env(built):
    J = built
    L = A.setup(J.lib())
    img = J.synth_image(W, H, seed=11)
    assert (img[..., 0] != img[..., 1]).mean() > 0.5  # a coloured body
    S = J.encode_rgb8(img)
    T = _grey(J, lambda: J.encode_rgb8(img))
    return J, L, img, S, T


def test_linear_grey_is_the_luminance_of_the_twin(env):
    J, L, img, S, T = env
    want = _luma_of_twin(L, S)
    got = _decode(L, T, (H, W, 1), 0, _grey_ce(8))[..., 0].astype(np.float64)
    err = np.abs(got - want).max()
    print("linear grey f32: max |got - want| = %.3g of max |want| = %.3g" % (err, np.abs(want).max()))
    assert err <= 4e-6 * np.abs(want).max()


def test_grey_body_with_equal_channels(env):
    """R = G = B in: the luminance of the twin's pixels (whose channels are then equal up to the codec's own error)."""
    J, L, img, S, T = env
    g = np.repeat(img[..., 1:2], 3, axis=2)
    want = _luma_of_twin(L, J.encode_rgb8(g))
    got = _decode(L, _grey(J, lambda: J.encode_rgb8(g)), (H, W, 1), 0, _grey_ce(8))[..., 0].astype(np.float64)
    assert np.abs(got - want).max() <= 4e-6 * np.abs(want).max()


def test_default_output_is_srgb_grey(env):
    J, L, img, S, T = env
    exp = _render(_luma_of_twin(L, S), "srgb")
    f32 = _decode(L, T, (H, W, 1), 0)[..., 0].astype(np.float64)
    print("sRGB grey f32: max error %.3g" % np.abs(f32 - exp).max())
    assert np.abs(f32 - exp).max() <= 2e-4
    u16 = _decode(L, T, (H, W, 1), 3)[..., 0].astype(np.float64)
    assert np.abs(u16 - np.clip(exp, 0, 1) * 65535).max() <= 2e-4 * 65535 + 1
    # three and four channels replicate (the matrix has three equal rows)
    rgb = _decode(L, T, (H, W, 3), 0).astype(np.float64)
    assert np.abs(rgb - exp[..., None]).max() <= 2e-4


@pytest.mark.parametrize("size", [(W, H), (601, 333)])
@pytest.mark.parametrize("epf,gab", [(1, 1), (1, 0), (2, 1), (2, 0)])
def test_gray8_from_the_filter_kernel(env, epf, gab, size):
    """GRAY8 comes from the one-channel form of the row-streaming filter kernel: sample for sample channel 0 of the same
    stream's RGB8 decode (the same expression on equal matrix rows), and within one level of the reading. The odd width
    runs both store alignments on alternate rows."""
    J, L = env[0], env[1]
    xs, ys = size
    img = J.synth_image(xs, ys, seed=11)
    kw = dict(epf_iters=epf, gab=gab)
    S = J.encode_rgb8(img, **kw)
    T = _grey(J, lambda: J.encode_rgb8(img, **kw))
    f = J.Frame(T)
    try:
        assert (f.info["epf_iters"], f.info["gab"]) == (epf, gab)
    finally:
        f.close()
    g8 = _decode(L, T, (ys, xs, 1), 2)[..., 0]
    rgb8 = _decode(L, T, (ys, xs, 3), 2)
    assert np.array_equal(g8, rgb8[..., 0])
    exp = np.clip(_render(_luma_of_twin(L, S, (ys, xs)), "srgb"), 0, 1) * 255
    err = np.abs(g8.astype(np.float64) - exp).max()
    print("GRAY8 epf %d gab %d %dx%d: max error %.4f levels" % (epf, gab, xs, ys, err))
    assert err <= 1.0 + 1e-3
    # RGB8 of a grey image: only the dither cell differs between the channels
    c = rgb8.astype(int)
    assert max(np.abs(c[..., 0] - c[..., 1]).max(), np.abs(c[..., 0] - c[..., 2]).max(), np.abs(c[..., 1] - c[..., 2]).max()) <= 1


def test_grey_with_alpha(env):
    """GA8 takes the generic writer: colour within one level of the reading, alpha exactly the RGBA twin's."""
    J, L, img = env[0], env[1], env[2]
    alpha = ((np.mgrid[0:H, 0:W][1] * 7 + np.mgrid[0:H, 0:W][0] * 3) % 256).astype(np.uint8)
    rgba = np.dstack([img, alpha])
    S = J.encode_rgba8(rgba)
    T = _grey(J, lambda: J.encode_rgba8(rgba))
    twin = _decode(L, S, (H, W, 4), 2)
    lin = _decode(L, S, (H, W, 4), 0, A.srgb_encoding(linear=True)).astype(np.float64)
    exp = np.clip(_render(lin[..., :3] @ LUMA, "srgb"), 0, 1) * 255
    ga = _decode(L, T, (H, W, 2), 2)
    assert np.array_equal(ga[..., 1], twin[..., 3])
    assert np.abs(ga[..., 0].astype(np.float64) - exp).max() <= 1.0 + 1e-3
    rgba8 = _decode(L, T, (H, W, 4), 2)
    assert np.array_equal(rgba8[..., 3], twin[..., 3])
    assert np.abs(rgba8[..., :3].astype(np.float64) - exp[..., None]).max() <= 1.0 + 1e-3


@pytest.mark.parametrize("name,kw,tf,intensity,inv_gamma", [
    ("gamma", dict(gamma=1 / 2.2), "gamma", 255.0, round(1e7 / 2.2) * 1e-7),
    ("709", dict(transfer_function=1), "709", 255.0, None),
    ("hlg", dict(transfer_function=18, intensity_target=1000.0), "hlg", 1000.0, None)])
def test_grey_gamma_709_hlg_streams(env, name, kw, tf, intensity, inv_gamma):
    """Grey streams in their own encoding (the generic writer): f32 against the reading of the twin's luminance, at
    test_gpu_color_encoding.py's tolerances (2e-4; 1e-3 on HLG's sqrt segment, whose slope at black is unbounded)."""
    J, L, img, S, _ = env
    T = _grey(J, lambda: J.encode_rgb8(img), **kw)
    y = _luma_of_twin(L, S) * (255.0 / intensity)
    lin = _decode(L, T, (H, W, 1), 0, _grey_ce(8))[..., 0].astype(np.float64)
    assert np.abs(lin - y).max() <= 4e-6 * np.abs(y).max()
    got = _decode(L, T, (H, W, 1), 0)[..., 0].astype(np.float64)
    exp = _render(y, tf, intensity, inv_gamma)
    tol = np.full(exp.shape, 2e-4)
    if tf == "hlg":
        tol[np.abs(exp) < 0.5] = 1e-3
    print("grey %s f32: max error %.3g" % (name, np.abs(got - exp).max()))
    assert (np.abs(got - exp) <= tol).all(), np.abs(got - exp).max()
    u8 = _decode(L, T, (H, W, 1), 2)[..., 0].astype(np.float64)
    assert np.abs(u8 - np.clip(exp, 0, 1) * 255).max() <= 1.0 + 1e-3


def test_icc_tagged_grey_stream(env):
    """A grey XYB image with an embedded ICC profile renders to sRGB grey, as ICC-tagged colour images render to sRGB."""
    J, L, img, S, T = env
    coded = open(os.path.join(ROOT, "tests", "golden", "ref_icc_test_profile.enc"), "rb").read()
    J.set_embedded_icc(coded)
    J.set_xyb_gray(True)
    try:
        TI = J.encode_rgb8(img)
    finally:
        J.set_xyb_gray(False)
        J.set_embedded_icc(None)
    exp = _render(_luma_of_twin(L, S), "srgb")
    f32 = _decode(L, TI, (H, W, 1), 0)[..., 0].astype(np.float64)
    assert np.abs(f32 - exp).max() <= 2e-4
    assert np.array_equal(_decode(L, TI, (H, W, 1), 2), _decode(L, T, (H, W, 1), 2))


def test_gray8_is_written_by_the_filter_kernel(env):
    """Which writer makes the pixels (jxlhip_debug_pixel_route): GRAY8 of a frame with one or two EPF iterations comes from
    the filter kernel's one-channel form (2), and is then the API's GRAY8; GA8, grey u16 and an oriented GRAY8 from the
    generic writer (0); RGB8 from the filter kernel (1)."""
    J, L, img, S, T = env
    want = _decode(L, T, (H, W, 1), 2)
    f = J.Frame(T)
    try:
        for fmt, orient, route in (((2, 1), 1, 2), ((2, 3), 1, 1), ((2, 2), 1, 0), ((3, 1), 1, 0), ((2, 1), 5, 0)):
            c = J.HipContext()
            try:
                c.set_output_format(*fmt)
                c.set_output_orientation(orient)
                c.upload(f)
                assert c.pixel_route() == route, (fmt, orient, c.pixel_route())
                if route == 2:
                    c.run_all()
                    c.sync()
                    assert np.array_equal(c.pixels(), want)
            finally:
                c.close()
    finally:
        f.close()


@pytest.mark.parametrize("name,tf_enum,gamma,tf,intensity,tol", [("pq", 16, 0.0, "pq", 10000.0, 5e-5)])
def test_grey_pq_colour_stage(env, name, tf_enum, gamma, tf, intensity, tol):
    """Grey PQ (intensity target 10000). The header reader refuses grey PQ, because the existing
    tests/test_color_encoding_host.py::test_grey_xyb_images_are_refused_where_they_were holds it to that for exactly this
    curve; so no stream reaches it and the colour stage itself is held, as
    test_gpu_color_encoding.py::test_kernel_stage_on_roundtrip_colours holds it for RGB and at its tolerance for the
    float32 powers of PQ (5e-5). The reading is the luminance of the RGB twin's matrix applied to the mixed signal,
    rendered in float64; nothing of the grey description enters it. A stream test like
    test_grey_gamma_709_hlg_streams belongs here once that refusal is lifted."""
    import ctypes
    import color_kat
    J, L, img, S, _ = env
    xyb = np.ascontiguousarray(color_kat.linear_srgb_to_xyb(color_kat.roundtrip_colors()), np.float32)
    mixed = C.xyb_to_mixed(xyb)
    twin = A.srgb_encoding()
    twin.transfer_function, twin.gamma = tf_enum, gamma
    m = np.array(A.color_output(L, twin, intensity, twin).matrix, np.float64).reshape(3, 3)
    grey = _grey_ce(tf_enum, gamma)
    t = A.color_output(L, grey, intensity, grey)
    ctx = J.HipContext()
    f = J.Frame(S)
    try:
        ctx.upload(f)  # (the opsin biases of a frame)
        out = np.empty((xyb.shape[1], 3), np.float32)
        assert L.jxlhip_debug_color_target(ctx._h, xyb.ctypes.data, xyb.shape[1], ctypes.byref(t), out.ctypes.data) == 0
    finally:
        f.close()
        ctx.close()
    y = LUMA @ (m @ mixed)
    exp = _render(y, tf, intensity, gamma if tf == "gamma" else None)
    err = np.abs(out.astype(np.float64) - exp[:, None]).max()
    print("grey %s colour stage: max error %.3g" % (name, err))
    assert err <= tol
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 0], out[:, 2])


def test_grey_xyb_modular_frame(env):
    J, L, img = env[0], env[1], env[2]
    part = img[:264, :320].copy()
    S = J.encode_lossless(part, J.MODULAR_XYB)
    J.set_xyb_gray(True)
    try:
        T = J.encode_lossless(part, J.MODULAR_XYB)
    finally:
        J.set_xyb_gray(False)
    assert S != T and len(S) - len(T) in range(-4, 5)
    want = _luma_of_twin(L, S, (264, 320))
    got = _decode(L, T, (264, 320, 1), 0, _grey_ce(8))[..., 0].astype(np.float64)
    assert np.abs(got - want).max() <= 4e-6 * np.abs(want).max()
    u8 = _decode(L, T, (264, 320, 1), 2)[..., 0].astype(np.float64)
    assert np.abs(u8 - np.clip(_render(want, "srgb"), 0, 1) * 255).max() <= 1.0 + 1e-3


def test_composed_still(env):
    """Two layers, the second blended (kBlend) through its alpha over the first. The luminance of a blend is the blend of
    the luminances only in linear light, and the canvas blends in the image's own transfer function: so both twins are
    tagged linear (S: linear sRGB, T: linear D65 grey). Float samples at the matrix bound, 8-bit ones (quantised and
    dithered) within one level of the same reading; the sRGB-tagged grey stream must decode to R = G = B."""
    J, L = env[0], env[1]
    cw, ch = 256, 200
    base, patch = J.synth_image(cw, ch, seed=31), J.synth_image(96, 64, seed=32)
    opaque = np.full((ch, cw), 255, np.uint8)
    ramp = ((np.mgrid[0:64, 0:96][1] * 255) // 95).astype(np.uint8)
    layers = [dict(img=np.dstack([base, opaque]), save_as=1),
              dict(img=np.dstack([patch, ramp]), x0=40, y0=30, mode=2, alpha_mode=2, source=1)]
    J.set_xyb_color_encoding(white_point=1, primaries=1, transfer_function=8)
    try:
        S = J.encode_layers(layers)
    finally:
        J.set_xyb_color_encoding(None)
    T = _grey(J, lambda: J.encode_layers(layers), transfer_function=8)
    twin = _decode(L, S, (ch, cw, 4), 0).astype(np.float64)
    want = twin[..., :3] @ LUMA
    ga = _decode(L, T, (ch, cw, 2), 0).astype(np.float64)
    assert np.array_equal(ga[..., 1], twin[..., 3])
    assert np.abs(ga[..., 0] - want).max() <= 4e-6 * np.abs(want).max()
    g = _decode(L, T, (ch, cw, 1), 0)[..., 0].astype(np.float64)
    assert np.abs(g - want).max() <= 4e-6 * np.abs(want).max()
    ga8 = _decode(L, T, (ch, cw, 2), 2).astype(np.float64)
    assert np.abs(ga8[..., 0] - np.clip(want, 0, 1) * 255).max() <= 1.0 + 1e-3
    assert np.abs(ga8[..., 1] - twin[..., 3] * 255).max() <= 1.0 + 1e-3
    g8 = _decode(L, T, (ch, cw, 1), 2)[..., 0].astype(np.float64)
    assert np.abs(g8 - np.clip(want, 0, 1) * 255).max() <= 1.0 + 1e-3
    # the sRGB target (blended in sRGB: no closed form from the twin's luminance)
    c = _decode(L, _grey(J, lambda: J.encode_layers(layers)), (ch, cw, 3), 2).astype(int)
    assert max(np.abs(c[..., 0] - c[..., 1]).max(), np.abs(c[..., 0] - c[..., 2]).max(), np.abs(c[..., 1] - c[..., 2]).max()) <= 1
    assert c.max() > 100


def test_oriented_gray8(env):
    """Orientation 5 (transposed): the generic writer; equal to channel 0 of the oriented RGB8 decode."""
    J, L, img = env[0], env[1], env[2]
    J.set_orientation(5)
    try:
        T = _grey(J, lambda: J.encode_rgb8(img))
    finally:
        J.set_orientation(1)
    g8 = _decode(L, T, (W, H, 1), 2)[..., 0]
    rgb8 = _decode(L, T, (W, H, 3), 2)
    assert np.array_equal(g8, rgb8[..., 0])
    plain = _decode(L, env[4], (H, W, 1), 2)[..., 0]
    assert np.abs(g8.astype(int) - plain.T.astype(int)).max() <= 1  # (the dither cell is taken after the flips)


_GUARD_CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
import libjxl_amd as J
J.set_xyb_color_encoding(white_point=1, transfer_function=13, gray=True)
data = J.encode_rgb8(J.synth_image(601, 333, seed=11))
f = J.Frame(data)
c = J.HipContext()
c.set_output_format(2, 1)
c.upload(f)
c.run_all()
c.sync()
print("guards", c.check_guards(), hashlib.sha256(c.pixels().tobytes()).hexdigest())
c.close()
f.close()
"""


def test_guard_bands_under_the_one_channel_writer(env):
    """JXLHIP_GUARD=1, fills 0xA5 and 0xFF, each in a fresh process: the one-channel writer of the odd-width image leaves
    the guard bands alone, and its bytes (1 per pixel in a buffer of xs * ys) are those of the API decode either way."""
    J, L = env[0], env[1]
    T = _grey(J, lambda: J.encode_rgb8(J.synth_image(601, 333, seed=11)))
    want = hashlib.sha256(_decode(L, T, (333, 601, 1), 2).tobytes()).hexdigest()
    for byte in ("0xA5", "0xFF"):
        e = dict(os.environ, JXLHIP_GUARD="1", JXLHIP_GUARD_BYTE=byte)
        r = subprocess.run([sys.executable, "-c", _GUARD_CHILD % ROOT], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("guards")][-1].split()
        assert line[1] == "0" and line[2] == want, (byte, line, want)
