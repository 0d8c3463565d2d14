"""XYB images tagged P3, Rec.2020 PQ / HLG, 709, DCI or a custom gamma, decoded on the GPU through the JxlDecoder API.
Every tagged stream T has an untagged twin S (the same XYB body): S is the oracle-pinned path, the tag must not change
the XYB decode (T to linear sRGB is S to linear sRGB, scaled by 255 / intensity target), and T's default output is the
float64 reading (tests/color_encoding_f64.py) of T's own linear sRGB pixels."""
import ctypes

import numpy as np
import pytest

import color_api as A
import color_encoding_f64 as C

pytestmark = pytest.mark.gpu

W, H = 600, 520  # several 256 x 256 groups, partial groups at both edges


@pytest.fixture(scope="module")
def env(built):
    J = built
    L = A.setup(J.lib())
    img = J.synth_image(W, H, seed=11)
    S = J.encode_rgb8(img)
    return J, L, img, S


def _linear(L, data, shape=(H, W, 3), desired=None):
    return A.decode(L, data, shape, 0, A.srgb_encoding(linear=True), desired=desired).astype(np.float64)


def _expected(name, lin_srgb, desired=None, linear_tf=False):
    """The reading of T's default output (or the original with a linear TF) from T's linear sRGB pixels [.., 3]."""
    _, p, w, tf, _ = A.ENCODINGS[name]
    flat = lin_srgb.reshape(-1, 3).T
    rgb = C.srgb_to_target(p, w) @ flat if (tuple(p) != C.SRGB or tuple(w) != C.D65) else flat
    if linear_tf:
        return rgb.T.reshape(lin_srgb.shape)
    out = C.render(rgb, tf, A.intensity(name), tf, desired=desired, p=p, w=w, inv_gamma=A.inv_gamma(name))
    return out.T.reshape(lin_srgb.shape)


def _tol(name, exp):
    """Per-sample bound in the encoded domain: 2e-4 (the float32 transcendentals); HLG's sqrt(3 x) segment (encoded < 0.5)
    has an unbounded slope at black, where float32 rounding of the linear value (1e-8 of summands ~0.3) alone moves the
    encoded value by up to sqrt(3e-8) = 1.7e-4, and the OOTF's luminance^-0.17 of such a value by more: 1e-3 there."""
    tol = np.full(exp.shape, 2e-4)
    if A.ENCODINGS[name][3] == "hlg":
        tol[np.abs(exp) < 0.5] = 1e-3
    return tol


def test_untagged_twin_is_the_oracle_path(env):
    import jxlo
    J, L, img, S = env
    got = A.decode(L, S, (H, W, 3), 2)
    ref = jxlo.Decoded(S, dumps=False).rgb8
    assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1


@pytest.mark.parametrize("name", sorted(A.ENCODINGS))
def test_tagged_stream(env, name):
    J, L, img, S = env
    T = A.tagged(J, name, lambda: J.encode_rgb8(img))
    it = A.intensity(name)
    lin_s, lin_t = _linear(L, S), _linear(L, T)
    # the tag does not change the XYB decode
    if it == 255.0:
        assert np.array_equal(lin_t, lin_s)
    else:
        want = lin_s * (255.0 / it)
        # (the scale sits in the matrix: each output is a sum of products up to ~11x its size, each rounded in float32,
        # so the difference is a few ulps of the summands rather than of the result)
        assert np.abs(lin_t - want).max() <= 4e-6 * np.abs(want).max()
    # default output: the image's own encoding
    exp = _expected(name, lin_t)
    tol = _tol(name, exp)
    f32 = A.decode(L, T, (H, W, 3), 0).astype(np.float64)
    assert (np.abs(f32 - exp) <= tol).all(), np.abs(f32 - exp).max()
    u16 = A.decode(L, T, (H, W, 3), 3).astype(np.float64)
    assert (np.abs(u16 - np.clip(exp, 0, 1) * 65535) <= tol * 65535 + 1).all()
    u8 = A.decode(L, T, (H, W, 3), 2).astype(np.float64)
    assert np.abs(u8 - np.clip(exp, 0, 1) * 255).max() <= 1.0 + 1e-3
    # the original encoding with a linear transfer function: the matrix alone
    d = A.Decoder(L, T)
    try:
        lin = A.copy_ce(d.profile(0))
        lin.transfer_function, lin.gamma = 8, 0.0
        assert d.set_output(lin) == 0
        got = d.decode(0).reshape(H, W, 3).astype(np.float64)
    finally:
        d.close()
    want = _expected(name, lin_t, linear_tf=True)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("desired", [255.0, 1000.0])
def test_pq_tone_mapping(env, desired):
    J, L, img, S = env
    T = A.tagged(J, "pq_10000", lambda: J.encode_rgb8(img))
    lin_t = _linear(L, T)
    got = A.decode(L, T, (H, W, 3), 0, desired=desired).astype(np.float64)
    exp = _expected("pq_10000", lin_t, desired=desired)
    assert np.abs(got - exp).max() <= 2e-4, np.abs(got - exp).max()


def test_hlg_ootf_to_srgb(env):
    J, L, img, S = env
    T = A.tagged(J, "hlg_1000", lambda: J.encode_rgb8(img))
    lin_t = _linear(L, T)  # (no tone mapping here: sRGB primaries, the image's own intensity target)
    got = A.decode(L, T, (H, W, 3), 0, A.srgb_encoding(), desired=255.0).astype(np.float64)
    flat = lin_t.reshape(-1, 3).T
    exp = C.render(flat, "hlg", 1000.0, "srgb", desired=255.0).T.reshape(H, W, 3)
    assert np.abs(got - exp).max() <= 2e-4, np.abs(got - exp).max()


def test_tone_mapped_image_with_a_dc_frame(env):
    """A still image whose DC image is a DC frame: decoded through the canvas, but neither frame is blended (the DC frame
    is kept before the colour transform, the image replaces the whole canvas), so the image is tone-mapped."""
    J, L, img, S = env
    T = A.tagged(J, "pq_10000", lambda: J.encode_with_dc_frame(img, dc_vardct=True))
    lin_t = _linear(L, T)
    got = A.decode(L, T, (H, W, 3), 0, desired=1000.0).astype(np.float64)
    exp = _expected("pq_10000", lin_t, desired=1000.0)
    assert np.abs(got - exp).max() <= 2e-4, np.abs(got - exp).max()


def test_tone_mapping_of_a_blended_frame_is_refused(env):
    """A layer blended over a saved base: the reference tone-maps such frames after blending, on encoded samples; refused."""
    J, L, img, S = env
    base, top = J.synth_image(256, 200, seed=31), J.synth_image(96, 64, seed=32)
    layers = [dict(img=base, save_as=1), dict(img=top, x0=40, y0=30, mode=1, source=1)]
    T = A.tagged(J, "pq_10000", lambda: J.encode_layers(layers))
    assert A.decode(L, T, (200, 256, 3), 0).shape == (200, 256, 3)  # (without tone mapping: decoded)
    d = A.Decoder(L, T)
    try:
        assert L.JxlDecoderSetDesiredIntensityTarget(d.dec, 1000.0) == 0
        st = L.JxlDecoderProcessInput(d.dec)  # (the hidden base frame, kept for reference, is decoded first)
        if st == 5:
            buf = np.zeros(200 * 256 * 3, np.float32)
            assert L.JxlDecoderSetImageOutBuffer(d.dec, ctypes.byref(A.Fmt(3, 0, 0, 0)), buf.ctypes.data, buf.nbytes) == 0
            st = L.JxlDecoderProcessInput(d.dec)
        assert st == 1 and b"tone mapping" in L.jxlamd_last_error()
    finally:
        d.close()


def test_upsampled_frame(env):
    J, L, img, S = env
    T = A.tagged(J, "pq_10000", lambda: J.encode_rgb8(img, upsampling=2))
    lin_t = _linear(L, T)
    got = A.decode(L, T, (H, W, 3), 0).astype(np.float64)
    assert np.abs(got - _expected("pq_10000", lin_t)).max() <= 2e-4


def _all_frames(L, data, shape, out=None):
    d = A.Decoder(L, data)
    frames = []
    try:
        assert d.status == 0x100
        if out is not None:
            assert d.set_output(out) == 0
        while len(frames) < 8:
            st = L.JxlDecoderProcessInput(d.dec)
            if st == 0:
                break
            assert st == 5, (st, L.jxlamd_last_error())
            fmt = A.Fmt(3, 0, 0, 0)
            buf = np.zeros(int(np.prod(shape)), np.float32)
            assert L.JxlDecoderSetImageOutBuffer(d.dec, ctypes.byref(fmt), buf.ctypes.data, buf.nbytes) == 0
            assert L.JxlDecoderProcessInput(d.dec) == 0x1000, L.jxlamd_last_error()
            frames.append(buf.reshape(shape).astype(np.float64))
    finally:
        d.close()
    return frames


def test_coalesced_animation_p3_pq(env):
    J, L, img, S = env
    frames = [J.synth_image(320, 264, seed=21), J.synth_image(320, 264, seed=22)]
    J.set_xyb_color_encoding(white_point=1, primaries=11, transfer_function=16, intensity_target=4000.0)
    try:
        T = J.encode_animation(frames, [1, 1])
    finally:
        J.set_xyb_color_encoding(None)
    lin = _all_frames(L, T, (264, 320, 3), A.srgb_encoding(linear=True))
    got = _all_frames(L, T, (264, 320, 3))
    assert len(lin) == len(got) == 2
    for lf, gf in zip(lin, got):
        flat = C.srgb_to_target(C.P3, C.D65) @ lf.reshape(-1, 3).T
        exp = C.render(flat, "pq", 4000.0, "pq", p=C.P3).T.reshape(gf.shape)
        assert np.abs(gf - exp).max() <= 2e-4


def test_xyb_modular_frame(env):
    J, L, img, S = env
    J.set_color_encoding(white_point=1, primaries=9, transfer_function=16)
    try:
        T = J.encode_lossless(img[:264, :320].copy(), J.MODULAR_XYB)
    finally:
        J.set_color_encoding(None)
    lin = _linear(L, T, (264, 320, 3))
    got = A.decode(L, T, (264, 320, 3), 0).astype(np.float64)
    flat = C.srgb_to_target(C.BT2100, C.D65) @ lin.reshape(-1, 3).T
    exp = C.render(flat, "pq", 255.0, "pq", p=C.BT2100).T.reshape(got.shape)
    assert np.abs(got - exp).max() <= 2e-4


def test_kernel_stage_on_roundtrip_colours(env):
    """jxlhip_debug_color_target on color_kat's XYB triples, every transfer function and both tone mappers."""
    import color_kat
    J, L, img, S = env
    rgb = color_kat.roundtrip_colors()
    xyb = np.ascontiguousarray(color_kat.linear_srgb_to_xyb(rgb), np.float32)
    mixed = C.xyb_to_mixed(xyb)
    ctx = J.HipContext()
    try:
        f = J.Frame(S)
        ctx.upload(f)  # (the opsin biases of a frame)
        cases = [("p3_srgb", None, None), ("pq_10000", None, None), ("pq_10000", None, 1000.0), ("hlg_1000", None, None),
                 ("hlg_1000", "srgb", 255.0), ("rec709", None, None), ("dci", None, None), ("custom_gamma", None, None)]
        for name, to, desired in cases:
            _, p, w, tf, _ = A.ENCODINGS[name]
            g, it = A.inv_gamma(name), A.intensity(name)
            src = _ce_of(name)
            dst = A.srgb_encoding() if to == "srgb" else src
            t = A.color_output(L, src, it, dst, desired or 0.0)
            out = np.empty((xyb.shape[1], 3), np.float32)
            assert L.jxlhip_debug_color_target(ctx._h, xyb.ctypes.data, xyb.shape[1], ctypes.byref(t), out.ctypes.data) == 0
            m = np.array(t.matrix, np.float64).reshape(3, 3)
            pp, ww = (C.SRGB, C.D65) if to == "srgb" else (p, w)
            exp = C.render(m @ mixed, tf, it, to or tf, desired=desired, p=pp, w=ww, inv_gamma=g).T
            # (PQ: the float32 powers; HLG: sqrt(3 x) at black turns float32 rounding noise of 1e-9 into 5e-5)
            tol = 2e-4 if to is None and tf == "hlg" else (5e-5 if tf == "pq" else 2e-5)
            assert np.abs(out - exp).max() <= tol, (name, np.abs(out - exp).max())
        f.close()
    finally:
        ctx.close()


def _ce_of(name):
    kw, p, w, tf, _ = A.ENCODINGS[name]
    ce = A.CE()
    ce.color_space, ce.white_point, ce.primaries = 0, kw["white_point"], kw["primaries"]
    ce.white_point_xy[:] = w
    ce.red[:], ce.green[:], ce.blue[:] = p[0:2], p[2:4], p[4:6]
    ce.transfer_function = 65535 if "gamma" in kw else kw["transfer_function"]
    ce.gamma = A.inv_gamma(name) if "gamma" in kw else 0.0
    ce.rendering_intent = 1
    return ce
