"""Grey XYB images on the host (no GPU): the colour stage's output description for a D65 grey image is the RGB one behind
three equal luminance rows (reference dec_xyb.cc:228-232), grey and RGB do not mix, the headers of a VarDCT stream tagged
(linear) sRGB grey parse, and the API hands out buffer sizes for 1 to 4 channels. The pixels: tests/test_gpu_grey_xyb.py."""
import ctypes

import numpy as np
import pytest

import color_api as A
import color_encoding_f64 as C

LUMA = np.array([0.2126, 0.7152, 0.0722])
XS, YS = 64, 48


@pytest.fixture(scope="module")
def L(built):
    return A.setup(built.lib())


def _ce(grey, tf=13, gamma=0.0, white_point=1, w=C.D65):
    ce = A.srgb_encoding()
    ce.color_space = 1 if grey else 0
    ce.white_point = white_point
    ce.white_point_xy[:] = w
    ce.transfer_function, ce.gamma = tf, gamma
    return ce


def _description(L, src, intensity, dst, desired=0.0):
    t = A.Target()
    r = L.jxlamd_color_output(ctypes.byref(src), intensity, ctypes.byref(dst), desired, None, ctypes.byref(t))
    return r, t


@pytest.mark.parametrize("intensity", [255.0, 1000.0])
@pytest.mark.parametrize("tf", [13, 8])
def test_grey_matrix_is_the_luminance_of_the_rgb_twin(L, intensity, tf):
    r, g = _description(L, _ce(True, tf), intensity, _ce(True, tf))
    assert r == 0, L.jxlamd_last_error()
    r, c = _description(L, _ce(False, tf), intensity, _ce(False, tf))
    assert r == 0
    M = np.array(c.matrix, np.float64).reshape(3, 3)
    G = np.array(g.matrix, np.float32).reshape(3, 3)
    assert np.array_equal(G[0], G[1]) and np.array_equal(G[0], G[2])
    assert abs(M[0, 0] - C.INV_OPSIN[0, 0] * 255.0 / intensity) < 1e-5 * abs(M[0, 0])  # (the twin carries the 255 / intensity scale)
    # three float32-rounded products of a double computation
    assert np.abs(G.astype(np.float64) - LUMA @ M).max() <= 1e-6 * np.abs(M).max()
    assert (g.tf, g.tone) == (c.tf, 0)
    assert np.abs(np.array(g.luminances) - LUMA).max() < 1e-6


@pytest.mark.parametrize("tf,gamma,want", [(16, 0.0, "pq"), (18, 0.0, "hlg"), (1, 0.0, "709"), (17, 0.0, "gamma"), (65535, 1 / 2.2, "gamma")])
def test_grey_transfer_functions_as_rgb(L, tf, gamma, want):
    r, g = _description(L, _ce(True, tf, gamma), 1000.0, _ce(True, tf, gamma))
    assert r == 0, L.jxlamd_last_error()
    r, c = _description(L, _ce(False, tf, gamma), 1000.0, _ce(False, tf, gamma))
    assert r == 0
    assert g.tf == c.tf == A.TF[want]
    for f in ("inv_gamma", "pq_display_scale", "hlg_exponent", "pre_scale", "post_scale", "tone"):
        assert getattr(g, f) == getattr(c, f), f
    G = np.array(g.matrix).reshape(3, 3)
    assert np.array_equal(G[0], G[1]) and np.array_equal(G[0], G[2])


def test_grey_pq_tone_mapping_description(L):
    """Tone mapping works on three equal channels with sRGB's luminances: the same mapper constants as the RGB twin's."""
    r, g = _description(L, _ce(True, 16), 10000.0, _ce(True, 16), 1000.0)
    assert r == 0
    r, c = _description(L, _ce(False, 16), 10000.0, _ce(False, 16), 1000.0)
    assert r == 0 and (g.tone, g.gamut_map) == (c.tone, c.gamut_map) == (1, 1)
    assert (g.tm_ks, g.tm_max_lum, g.tm_normalizer) == (c.tm_ks, c.tm_max_lum, c.tm_normalizer)
    assert np.abs(np.array(g.luminances) - LUMA).max() < 1e-6


def test_grey_and_rgb_do_not_mix(L):
    assert _description(L, _ce(True), 255.0, _ce(False))[0] != 0
    assert _description(L, _ce(False), 255.0, _ce(True))[0] != 0
    # a grey white point other than D65 (the reference falls back to linear grey there: a deviation)
    e = _ce(True, white_point=10, w=C.E_WHITE)
    assert _description(L, e, 255.0, e)[0] != 0


def _grey_stream(J, **kw):
    J.set_xyb_color_encoding(**dict(dict(white_point=1, transfer_function=13, gray=True), **kw))
    try:
        return J.encode_rgb8(J.synth_image(XS, YS, seed=5))
    finally:
        J.set_xyb_color_encoding(None)


def test_gray_tag_only_changes_the_header(built):
    J = built
    plain = J.encode_rgb8(J.synth_image(XS, YS, seed=5))
    J.set_xyb_color_encoding(white_point=1, transfer_function=13)
    try:
        rgb = J.encode_rgb8(J.synth_image(XS, YS, seed=5))
    finally:
        J.set_xyb_color_encoding(None)
    grey = _grey_stream(J)
    assert grey != rgb and grey != plain
    assert J.encode_rgb8(J.synth_image(XS, YS, seed=5)) == plain  # (the switch is off again)
    n = min(len(grey), len(plain)) - 64
    assert grey[-n:] == plain[-n:]  # the body behind the (byte-aligned) headers is the untagged twin's


def test_grey_vardct_headers_and_buffer_sizes(built, L):
    J = built
    data = _grey_stream(J)
    J.Frame(data).close()  # (the host front-end parses the frame)
    d = A.Decoder(L, data)
    try:
        assert d.status == 0x100
        info = (ctypes.c_uint8 * 512)()
        assert L.JxlDecoderGetBasicInfo(d.dec, info) == 0
        assert ctypes.c_uint32.from_buffer(info, 52).value == 1  # num_color_channels
        for target in (0, 1):
            ce = d.profile(target)
            assert (ce.color_space, ce.white_point, ce.transfer_function) == (1, 1, 13)
        size = ctypes.c_size_t()
        for nc in (1, 2, 3, 4):
            for data_type, nbytes in ((0, 4), (2, 1), (3, 2)):
                assert L.JxlDecoderImageOutBufferSize(d.dec, ctypes.byref(A.Fmt(nc, data_type, 0, 0)), ctypes.byref(size)) == 0
                assert size.value == XS * YS * nc * nbytes
        # the outputs of a grey image are grey: (linear) sRGB grey, or its own encoding
        assert d.set_output(A.srgb_encoding()) == 1
        assert d.set_output(_ce(True, 8)) == 0 and d.profile(1).transfer_function == 8
        assert d.profile(1).color_space == 1 and d.profile(0).transfer_function == 13
    finally:
        d.close()


def test_grey_with_white_point_e_is_refused(built, L):
    """The reference falls back to linear grey there (dec_xyb.cc:137-140,160-164): refused with the headers."""
    J = built
    data = _grey_stream(J, white_point=10)
    d = A.Decoder(L, data)
    try:
        assert d.status == 1  # JXL_DEC_ERROR with the headers
    finally:
        d.close()
    with pytest.raises(J.JxlAmdError, match="colour space other than D65 grey"):
        J.Frame(data)


@pytest.mark.parametrize("kw,tf", [(dict(gamma=1 / 2.2), 65535), (dict(transfer_function=1), 1), (dict(transfer_function=17), 17),
                                   (dict(transfer_function=18, intensity_target=1000.0), 18)])
def test_grey_curves_are_admitted(built, L, kw, tf):
    """D65 grey with a gamma, 709, DCI or HLG: the headers parse and both profiles report the image's own encoding."""
    J = built
    data = _grey_stream(J, **kw)
    J.Frame(data).close()
    d = A.Decoder(L, data)
    try:
        assert d.status == 0x100
        for target in (0, 1):
            ce = d.profile(target)
            assert (ce.color_space, ce.white_point, ce.transfer_function) == (1, 1, tf)
        if tf == 65535:
            assert abs(d.profile(1).gamma - 1 / 2.2) < 1e-6
        assert d.set_output(_ce(True, 13)) == 0 and d.profile(1).transfer_function == 13
    finally:
        d.close()


def test_icc_tagged_grey_xyb_reports_srgb_grey(built, L):
    """An embedded ICC profile on a grey XYB image: the original profile is the ICC one, the pixels are sRGB grey."""
    import os
    J = built
    root = os.path.dirname(os.path.abspath(__file__))
    coded = open(os.path.join(root, "golden", "ref_icc_test_profile.enc"), "rb").read()
    J.set_embedded_icc(coded)
    J.set_xyb_gray(True)
    try:
        data = J.encode_rgb8(J.synth_image(XS, YS, seed=5))
    finally:
        J.set_xyb_gray(False)
        J.set_embedded_icc(None)
    J.Frame(data).close()
    d = A.Decoder(L, data)
    try:
        assert d.status == 0x100
        info = (ctypes.c_uint8 * 512)()
        assert L.JxlDecoderGetBasicInfo(d.dec, info) == 0
        assert ctypes.c_uint32.from_buffer(info, 52).value == 1  # num_color_channels
        ce = A.CE()
        assert L.JxlDecoderGetColorAsEncodedProfile(d.dec, 0, ctypes.byref(ce)) == 1  # ORIGINAL: the ICC form only
        ce = d.profile(1)
        assert (ce.color_space, ce.white_point, ce.transfer_function) == (1, 1, 13)
        assert d.set_output(_ce(True, 8)) == 0 and d.profile(1).transfer_function == 8
        size = ctypes.c_size_t()
        assert L.JxlDecoderImageOutBufferSize(d.dec, ctypes.byref(A.Fmt(1, 2, 0, 0)), ctypes.byref(size)) == 0
        assert size.value == XS * YS
    finally:
        d.close()


def test_linear_grey_header(built, L):
    J = built
    d = A.Decoder(L, _grey_stream(J, transfer_function=8))
    try:
        assert d.status == 0x100
        for target in (0, 1):
            ce = d.profile(target)
            assert (ce.color_space, ce.white_point, ce.transfer_function) == (1, 1, 8)
        assert d.set_output(_ce(True, 13)) == 0  # towards sRGB grey: the colour space of the header stays
        ce = d.profile(1)
        assert (ce.color_space, ce.white_point, ce.transfer_function) == (1, 1, 13)
    finally:
        d.close()


def test_grey_xyb_modular_frame_parses(built):
    """An XYB Modular frame of a grey image has three colour channels (dec_modular.cc: one only without a colour transform)."""
    J = built
    img = J.synth_image(XS, YS, seed=5)
    J.set_xyb_gray(True)
    try:
        data = J.encode_lossless(img, J.MODULAR_XYB)
    finally:
        J.set_xyb_gray(False)
    assert data != J.encode_lossless(img, J.MODULAR_XYB)
    f = J.ModFrame(data)
    try:
        assert f.info["num_color"] == 3
    finally:
        f.close()
