"""XYB images tagged with an enum colour encoding other than (linear) sRGB, on the host (no GPU): the headers parse, the
API reports and gates the output encoding, and the colour stage's output description (jxlamd_color_output) matches the
float64 reading of tests/color_encoding_f64.py, which is itself held to constants published outside the reference."""
import ctypes

import numpy as np
import pytest

import color_api as A
import color_encoding_f64 as C


@pytest.fixture(scope="module")
def L(built):
    return A.setup(built.lib())


def _stream(J, name):
    return A.tagged(J, name, lambda: J.encode_rgb8(J.synth_image(64, 48, seed=5)))


# ---- the reading against published numbers
def test_reading_holds_published_constants():
    # ITU-R BT.2087: linear BT.709 -> BT.2020 (same white point)
    bt2087 = np.array([[0.6274, 0.3293, 0.0433], [0.0691, 0.9195, 0.0114], [0.0164, 0.0880, 0.8956]])
    assert np.abs(C.srgb_to_target(C.BT2100, C.D65) - bt2087).max() < 1e-3
    # linear sRGB -> Display P3
    p3 = np.array([[0.8225, 0.1774, 0.0], [0.0332, 0.9669, 0.0], [0.0171, 0.0724, 0.9108]])
    assert np.abs(C.srgb_to_target(C.P3, C.D65) - p3).max() < 1e-3
    # SMPTE ST 2084
    assert np.abs(C.pq_encode_nits(np.array([100.0, 1000.0, 10000.0])) - [0.5081, 0.7518, 1.0]).max() < 1e-4
    assert np.abs(C.pq_decode_nits(C.pq_encode_nits(np.array([0.5, 100.0, 4000.0]))) - [0.5, 100.0, 4000.0]).max() < 1e-9 * 4000
    # BT.2100 HLG
    assert np.abs(C.hlg_encode(np.array([1 / 12, 1.0])) - [0.5, 1.0]).max() < 1e-6
    # a matrix towards the same primaries is the identity; luminances of sRGB are BT.709's
    assert np.abs(C.srgb_to_target(C.SRGB, C.D65) - np.eye(3)).max() < 1e-12
    assert np.abs(C.luminances(C.SRGB, C.D65) - [0.2126, 0.7152, 0.0722]).max() < 1e-4


# ---- headers
@pytest.mark.parametrize("name", sorted(A.ENCODINGS))
def test_tagged_xyb_header_parses(built, L, name):
    J = built
    data = _stream(J, name)
    J.Frame(data).close()  # (raised "unsupported: XYB image in a colour space other than (linear) sRGB" before)
    kw, p, w, tf, _ = A.ENCODINGS[name]
    d = A.Decoder(L, data)
    try:
        assert d.status == 0x100
        for target in (0, 1):  # ORIGINAL, DATA: the default output of an XYB image is its own encoding
            ce = d.profile(target)
            assert (ce.white_point, ce.primaries) == (kw["white_point"], kw["primaries"])
            assert ce.transfer_function == (65535 if "gamma" in kw else kw["transfer_function"])
            assert np.allclose(list(ce.white_point_xy), w, atol=1e-6)
            assert np.allclose(list(ce.red) + list(ce.green) + list(ce.blue), p, atol=1e-6)
        assert abs(d.basic_intensity() - A.intensity(name)) < 1e-3
    finally:
        d.close()


def test_untagged_streams_do_not_change(built):
    """With the switch off the encoder writes what it wrote before (the fixtures depend on it)."""
    J = built
    img = J.synth_image(64, 48, seed=5)
    before = J.encode_rgb8(img)
    J.set_xyb_color_encoding(**A.ENCODINGS["pq_10000"][0])
    tagged = J.encode_rgb8(img)
    J.set_xyb_color_encoding(None)
    assert J.encode_rgb8(img) == before and tagged != before


def _grey_xyb_header(transfer_function=13):
    """A codestream that declares a grey XYB image of 8 x 8 pixels (image_metadata.cc, color_encoding_internal.cc) and
    then a default frame whose sections are empty."""
    bits = []

    def w(n, v):
        bits.extend((v >> i) & 1 for i in range(n))

    w(16, 0x0AFF)
    w(1, 1); w(5, 0); w(3, 1)  # small size: 8 x 8 (ratio 1)
    w(1, 0); w(1, 0)  # metadata not all_default, no extra fields
    w(1, 0); w(2, 0)  # 8-bit integer samples
    w(1, 1); w(2, 0)  # modular_16_bit, no extra channels
    w(1, 1)  # xyb_encoded
    w(1, 0); w(1, 0); w(2, 1)  # colour encoding: not all_default, no ICC, grey
    w(2, 1)  # D65
    w(1, 0); w(2, 2); w(4, transfer_function - 2)  # transfer function (enum selector 2: 4 bits + 2)
    w(2, 1)  # rendering intent relative
    w(2, 0)  # no extensions
    w(1, 1)  # default transform data
    bits += [0] * (-len(bits) % 8)
    w(1, 1)  # frame header all_default
    bits += [0] * (-len(bits) % 8) + [0] * 64
    return bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))


def test_grey_xyb_images_are_refused_where_they_were(built, L):
    """A grey XYB image in sRGB gets its header events (basic info, colour encoding) and is refused at the pixels, as
    before; one in another colour encoding is still refused with the headers."""
    data = _grey_xyb_header()
    d = A.Decoder(L, data)
    try:
        assert d.status == 0x100  # (BASIC_INFO came first: A.Decoder steps over it)
        ce = d.profile(0)
        assert (ce.color_space, ce.white_point, ce.transfer_function) == (1, 1, 13)
        assert d.profile(1).color_space == 1
        st = L.JxlDecoderProcessInput(d.dec)
        if st == 5:  # NEED_IMAGE_OUT_BUFFER: no output format exists for a grey VarDCT image here
            size = ctypes.c_size_t()
            for nc in (1, 3):
                assert L.JxlDecoderImageOutBufferSize(d.dec, ctypes.byref(A.Fmt(nc, 0, 0, 0)), ctypes.byref(size)) == 1
        else:
            assert st == 1, st  # JXL_DEC_ERROR
    finally:
        d.close()
    d = A.Decoder(L, _grey_xyb_header(transfer_function=16))
    try:
        assert d.status == 1  # JXL_DEC_ERROR before any event
    finally:
        d.close()
    with pytest.raises(built.JxlAmdError, match="colour space other than"):
        built.Frame(_grey_xyb_header(transfer_function=16))


# ---- JxlDecoderSetOutputColorProfile / SetDesiredIntensityTarget
def test_output_profile_gate(built, L):
    J = built
    d = A.Decoder(L, _stream(J, "pq_10000"))
    try:
        orig = d.profile(0)
        bad = A.copy_ce(orig)
        bad.primaries, bad.red[:], bad.green[:], bad.blue[:] = 11, C.P3[0:2], C.P3[2:4], C.P3[4:6]
        assert d.set_output(bad) == 1  # another enum target: refused here (the reference would render it)
        bad = A.copy_ce(orig)
        bad.transfer_function = 18
        assert d.set_output(bad) == 1
        assert d.profile(1).transfer_function == 16  # a refused call changes nothing
        # (c) the original with a linear transfer function
        lin = A.copy_ce(orig)
        lin.transfer_function = 8
        assert d.set_output(lin) == 0
        data = d.profile(1)
        assert (data.primaries, data.transfer_function) == (9, 8) and d.profile(0).transfer_function == 16
        # (b) the original itself, whatever the rendering intent
        same = A.copy_ce(orig)
        same.rendering_intent = 3
        assert d.set_output(same) == 0 and d.profile(1).transfer_function == 16
        # (a) sRGB / linear sRGB: DATA reports sRGB primaries and white point
        assert d.set_output(A.srgb_encoding(linear=True)) == 0
        data = d.profile(1)
        assert (data.white_point, data.primaries, data.transfer_function) == (1, 1, 8)
        assert np.allclose(list(data.red), C.SRGB[0:2])
        assert d.set_output(A.srgb_encoding()) == 0 and d.profile(1).transfer_function == 13
        assert d.profile(0).primaries == 9
    finally:
        d.close()
    # an sRGB image: PQ output stays refused (tests/test_host.py holds the same), its DATA profile is as before
    d = A.Decoder(L, J.encode_rgb8(J.synth_image(64, 48)))
    try:
        ce = d.profile(1)
        assert (ce.primaries, ce.transfer_function) == (1, 13) and tuple(ce.red) == C.SRGB[0:2]
        ce.transfer_function = 16
        assert d.set_output(ce) == 1
    finally:
        d.close()


def test_desired_intensity_target(built, L):
    J = built
    d = A.Decoder(L, _stream(J, "pq_10000"))
    try:
        assert abs(d.basic_intensity() - 10000.0) < 1e-3
        assert L.JxlDecoderSetDesiredIntensityTarget(d.dec, -1.0) == 1
        assert L.JxlDecoderSetDesiredIntensityTarget(d.dec, 300.0) == 0
        assert abs(d.basic_intensity() - 300.0) < 1e-3
        assert L.JxlDecoderSetDesiredIntensityTarget(d.dec, 0.0) == 0  # 0: the image's again
        assert abs(d.basic_intensity() - 10000.0) < 1e-3
    finally:
        d.close()


# ---- the host output description against the reading
def _ce(p, w, tf, gamma=None):
    ce = CE_from(p, w)
    ce.transfer_function = {"linear": 8, "srgb": 13, "pq": 16, "hlg": 18, "709": 1}.get(tf, 65535)
    if ce.transfer_function == 65535:
        ce.gamma = gamma
    return ce


def CE_from(p, w):
    ce = A.CE()
    ce.color_space = 0
    ce.white_point = {C.D65: 1, C.DCI_WHITE: 11, C.E_WHITE: 10}.get(tuple(w), 2)
    ce.primaries = {C.SRGB: 1, C.BT2100: 9, C.P3: 11}.get(tuple(p), 2)
    ce.white_point_xy[:] = w
    ce.red[:], ce.green[:], ce.blue[:] = p[0:2], p[2:4], p[4:6]
    ce.rendering_intent = 1
    return ce


def _rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize("name", sorted(A.ENCODINGS))
def test_output_description_matches_reading(L, name):
    _, p, w, tf, _ = A.ENCODINGS[name]
    it = A.intensity(name)
    g = A.inv_gamma(name)
    src = _ce(p, w, tf, g)
    if name == "dci":
        src.transfer_function = 17
    t = A.color_output(L, src, it, src)
    assert t.tf == A.TF[tf] and t.tone == 0
    want = C.output_matrix(p, w, it)
    assert _rel(np.array(t.matrix).reshape(3, 3), want) < 1e-6
    lum = C.luminances(p, w) if tuple(p) != C.SRGB else np.array([0.2126, 0.7152, 0.0722])
    assert _rel(t.luminances, lum) < 1e-6
    if tf == "gamma":
        assert abs(t.inv_gamma - g) < 1e-6 * g
    if tf == "pq":
        assert abs(t.pq_display_scale - it / 10000) < 1e-7
    if tf == "hlg":
        assert abs(t.hlg_exponent - C.hlg_to_scene_exponent(it)) < 1e-6
    # (a) linear sRGB of the same image: the image's own matrix, sRGB luminances, no tone mapping
    t = A.color_output(L, src, it, A.srgb_encoding(linear=True))
    assert t.tf == A.TF["linear"] and t.tone == 0
    assert _rel(np.array(t.matrix).reshape(3, 3), C.INV_OPSIN * (255.0 / it)) < 1e-6


def test_tone_mapping_description(L):
    src = _ce(C.BT2100, C.D65, "pq")
    for desired in (255.0, 1000.0):
        t = A.color_output(L, src, 10000.0, src, desired)
        assert (t.tf, t.tone, t.gamut_map) == (A.TF["pq"], 1, 1)
        assert abs(t.pre_scale - 1.0) < 1e-7 and abs(t.post_scale - desired / 10000) < 1e-6 * desired / 10000  # 10000 / orig, desired / 10000
        pq_min = C.pq_encode_nits(0.0)
        pq_range = C.pq_encode_nits(10000.0) - pq_min
        max_lum = (C.pq_encode_nits(desired) - pq_min) / pq_range
        for got, want in ((t.tm_pq_min, pq_min), (t.tm_pq_range, pq_range), (t.tm_max_lum, max_lum), (t.tm_ks, 1.5 * max_lum - 0.5),
                          (t.tm_normalizer, 10000.0 / desired), (t.tm_source_peak, 10000.0), (t.tm_target_peak, desired)):
            assert abs(got - want) <= 1e-6 * abs(want) + 1e-12, (got, want)
        assert _rel(t.luminances, C.luminances(C.BT2100, C.D65)) < 1e-6
    # desired above the image's: no tone mapping of a PQ image
    assert A.color_output(L, src, 1000.0, src, 4000.0).tone == 0
    # HLG rendered to sRGB for a 255 cd/m2 display: the OOTF, with gamut mapping (its exponent is negative)
    hlg = _ce(C.BT2100, C.D65, "hlg")
    t = A.color_output(L, hlg, 1000.0, A.srgb_encoding(), 255.0)
    e = C.hlg_tone_exponent(1000.0, 255.0)
    assert (t.tf, t.tone, t.gamut_map) == (A.TF["srgb"], 2, 1) and abs(t.tone_exponent - e) < 1e-6
    assert abs(t.pre_scale - 1) < 1e-9 and abs(t.post_scale - 1) < 1e-9
    # HLG to HLG: the output curve's OOTF for the desired display, no tone mapper
    t = A.color_output(L, hlg, 1000.0, hlg, 400.0)
    assert t.tone == 0 and abs(t.hlg_exponent - C.hlg_to_scene_exponent(400.0)) < 1e-6
