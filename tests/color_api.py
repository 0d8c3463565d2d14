"""ctypes access to the colour-encoding surface of libjxl_amd for the tests: JxlColorEncoding / JxlHipColorTarget mirrors,
tagged test streams, and a JxlDecoder run with an output profile and a desired intensity target."""
import ctypes

import numpy as np

import color_encoding_f64 as C


class CE(ctypes.Structure):  # JxlColorEncoding
    _fields_ = [("color_space", ctypes.c_int), ("white_point", ctypes.c_int), ("white_point_xy", ctypes.c_double * 2),
                ("primaries", ctypes.c_int), ("red", ctypes.c_double * 2), ("green", ctypes.c_double * 2),
                ("blue", ctypes.c_double * 2), ("transfer_function", ctypes.c_int), ("gamma", ctypes.c_double),
                ("rendering_intent", ctypes.c_int)]


class Target(ctypes.Structure):  # JxlHipColorTarget
    _fields_ = [("matrix", ctypes.c_float * 9), ("tf", ctypes.c_uint32), ("tone", ctypes.c_uint32), ("gamut_map", ctypes.c_uint32),
                ("luminances", ctypes.c_float * 3), ("pre_scale", ctypes.c_float), ("post_scale", ctypes.c_float),
                ("pq_display_scale", ctypes.c_float), ("inv_gamma", ctypes.c_float), ("hlg_exponent", ctypes.c_float),
                ("tone_exponent", ctypes.c_float)] + [(n, ctypes.c_float) for n in (
                    "tm_source_peak", "tm_target_peak", "tm_pq_min", "tm_pq_range", "tm_inv_pq_range", "tm_min_lum", "tm_max_lum",
                    "tm_ks", "tm_inv_one_minus_ks", "tm_normalizer", "tm_inv_target_peak")]


class Fmt(ctypes.Structure):  # JxlPixelFormat
    _fields_ = [("num_channels", ctypes.c_uint32), ("data_type", ctypes.c_int), ("endianness", ctypes.c_int), ("align", ctypes.c_size_t)]


TF = {"linear": 1, "srgb": 2, "pq": 3, "hlg": 4, "709": 5, "gamma": 6}
ENUM_TF = {1: "709", 8: "linear", 13: "srgb", 16: "pq", 17: "gamma", 18: "hlg"}

# The encodings of the issue: name -> (set_xyb_color_encoding keywords, reading's primaries, white, tf, inv_gamma)
CUSTOM_XY = [0.3, 0.32, 0.66, 0.31, 0.28, 0.62, 0.16, 0.07]  # white, red, green, blue
ENCODINGS = {
    "p3_srgb": (dict(white_point=1, primaries=11, transfer_function=13), C.P3, C.D65, "srgb", None),
    "pq_10000": (dict(white_point=1, primaries=9, transfer_function=16, intensity_target=10000.0), C.BT2100, C.D65, "pq", None),
    "hlg_1000": (dict(white_point=1, primaries=9, transfer_function=18, intensity_target=1000.0), C.BT2100, C.D65, "hlg", None),
    "rec709": (dict(white_point=1, primaries=1, transfer_function=1), C.SRGB, C.D65, "709", None),
    "dci": (dict(white_point=11, primaries=11, transfer_function=17), C.P3, C.DCI_WHITE, "gamma", 1 / 2.6),
    "custom_gamma": (dict(white_point=2, primaries=2, gamma=1 / 2.2, xy=CUSTOM_XY), tuple(CUSTOM_XY[2:]), tuple(CUSTOM_XY[:2]),
                     "gamma", None),
}


def intensity(name):
    return ENCODINGS[name][0].get("intensity_target", 255.0)


def inv_gamma(name):
    kw, _, _, _, g = ENCODINGS[name]
    if g is not None:
        return g
    return round(kw["gamma"] * 1e7) * 1e-7 if "gamma" in kw else None


def tagged(J, name, encode):
    """encode() with the encoding `name` declared on the VarDCT header (the same XYB body as without it)."""
    J.set_xyb_color_encoding(**ENCODINGS[name][0])
    try:
        return encode()
    finally:
        J.set_xyb_color_encoding(None)


def setup(L):
    vp = ctypes.c_void_p
    L.JxlDecoderCreate.restype = vp
    L.JxlDecoderCreate.argtypes = [vp]
    for n in ("JxlDecoderDestroy", "JxlDecoderProcessInput", "JxlDecoderCloseInput"):
        getattr(L, n).argtypes = [vp]
    L.JxlDecoderSubscribeEvents.argtypes = [vp, ctypes.c_int]
    L.JxlDecoderSetInput.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    L.JxlDecoderGetColorAsEncodedProfile.argtypes = [vp, ctypes.c_int, ctypes.POINTER(CE)]
    L.JxlDecoderSetOutputColorProfile.argtypes = [vp, ctypes.POINTER(CE), vp, ctypes.c_size_t]
    L.JxlDecoderSetDesiredIntensityTarget.argtypes = [vp, ctypes.c_float]
    L.JxlDecoderGetBasicInfo.argtypes = [vp, vp]
    L.JxlDecoderImageOutBufferSize.argtypes = [vp, ctypes.POINTER(Fmt), ctypes.POINTER(ctypes.c_size_t)]
    L.JxlDecoderSetImageOutBuffer.argtypes = [vp, ctypes.POINTER(Fmt), vp, ctypes.c_size_t]
    L.jxlamd_color_output.argtypes = [ctypes.POINTER(CE), ctypes.c_float, ctypes.POINTER(CE), ctypes.c_float, vp, ctypes.POINTER(Target)]
    L.jxlhip_debug_color_target.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(Target), vp]
    return L


def srgb_encoding(linear=False):
    ce = CE()
    ce.color_space, ce.white_point, ce.primaries = 0, 1, 1
    ce.white_point_xy[:] = C.D65
    ce.red[:], ce.green[:], ce.blue[:] = C.SRGB[0:2], C.SRGB[2:4], C.SRGB[4:6]
    ce.transfer_function = 8 if linear else 13
    ce.rendering_intent = 1
    return ce


def copy_ce(ce):
    out = CE()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(ce), ctypes.sizeof(CE))
    return out


def color_output(L, src, src_intensity, dst, desired=0.0):
    t = Target()
    assert L.jxlamd_color_output(ctypes.byref(src), src_intensity, ctypes.byref(dst), desired, None, ctypes.byref(t)) == 0
    return t


class Decoder:
    """A JxlDecoder stopped at the colour-encoding event (pixels: decode())."""

    def __init__(self, L, data):
        self.L, self.data = L, data
        self.dec = L.JxlDecoderCreate(None)
        assert L.JxlDecoderSubscribeEvents(self.dec, 0x40 | 0x100 | 0x1000) == 0
        L.JxlDecoderSetInput(self.dec, data, len(data))
        L.JxlDecoderCloseInput(self.dec)
        self.status = L.JxlDecoderProcessInput(self.dec)
        if self.status == 0x40:
            self.status = L.JxlDecoderProcessInput(self.dec)

    def profile(self, target):
        ce = CE()
        assert self.L.JxlDecoderGetColorAsEncodedProfile(self.dec, target, ctypes.byref(ce)) == 0
        return ce

    def set_output(self, ce):
        return self.L.JxlDecoderSetOutputColorProfile(self.dec, ctypes.byref(ce), None, 0)

    def basic_intensity(self):
        buf = (ctypes.c_uint8 * 512)()
        assert self.L.JxlDecoderGetBasicInfo(self.dec, buf) == 0
        return ctypes.c_float.from_buffer(buf, 20).value

    def decode(self, data_type=0, nc=3):
        """The image as [ys, xs, nc] float32 / uint16 / uint8 (data_type 0 / 3 / 2)."""
        L = self.L
        st = L.JxlDecoderProcessInput(self.dec)
        assert st == 5, (st, L.jxlamd_last_error())
        fmt = Fmt(nc, data_type, 0, 0)
        size = ctypes.c_size_t()
        assert L.JxlDecoderImageOutBufferSize(self.dec, ctypes.byref(fmt), ctypes.byref(size)) == 0
        dt = {0: np.float32, 2: np.uint8, 3: np.uint16}[data_type]
        buf = np.zeros(size.value // np.dtype(dt).itemsize, dt)
        assert L.JxlDecoderSetImageOutBuffer(self.dec, ctypes.byref(fmt), buf.ctypes.data, size.value) == 0
        st = L.JxlDecoderProcessInput(self.dec)
        assert st == 0x1000, (st, L.jxlamd_last_error())
        return buf

    def close(self):
        if self.dec:
            self.L.JxlDecoderDestroy(self.dec)
            self.dec = None


def decode(L, data, shape, data_type=0, out=None, desired=None):
    """Decodes `data` through the API: out = a CE to SetOutputColorProfile (None: the default), desired = an intensity target."""
    d = Decoder(L, data)
    try:
        assert d.status == 0x100, d.status
        if out is not None:
            assert d.set_output(out) == 0
        if desired is not None:
            assert L.JxlDecoderSetDesiredIntensityTarget(d.dec, desired) == 0
        return d.decode(data_type).reshape(shape)
    finally:
        d.close()
