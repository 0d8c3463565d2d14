"""An independent float64 reading of how the reference renders an XYB image to an enum colour encoding without a CMS:
lib/jxl/cms/jxl_cms_internal.h:43-126 (PrimariesToXYZ, Bradford AdaptToXYZD50), lib/jxl/dec_xyb.cc:181-229 (the inverse
opsin matrix towards the target primaries, luminances), render_pipeline/stage_from_linear.cc:37-99 with the curves of the
standards (IEC 61966-2-1 sRGB, SMPTE ST 2084 PQ, BT.2100 HLG, BT.709, a pure gamma), stage_tone_mapping.cc:30-120 and
cms/tone_mapping.h:23-175 (Rec2408ToneMapperBase::ToneMap, HlgOOTF_Base::Apply, GamutMapScalar). No decoder produced any
of these numbers; the reading itself is held to constants published outside the reference (test_color_encoding_host.py)."""
import numpy as np

# white points and primaries of the enum values (xy)
D65 = (0.3127, 0.3290)
DCI_WHITE = (0.314, 0.351)
E_WHITE = (1 / 3, 1 / 3)
SRGB = (0.639998686, 0.330010138, 0.300003784, 0.600003357, 0.150002046, 0.059997204)
BT2100 = (0.708, 0.292, 0.170, 0.797, 0.131, 0.046)
P3 = (0.680, 0.320, 0.265, 0.690, 0.150, 0.060)
WHITE = {1: D65, 10: E_WHITE, 11: DCI_WHITE}
PRIMARIES = {1: SRGB, 9: BT2100, 11: P3}

# XYB -> linear sRGB of the default OpsinInverseMatrix (opsin_params.h) and its bias
INV_OPSIN = np.array([[11.031566901960783, -9.866943921568629, -0.16462299647058826],
                      [-3.254147380392157, 4.418770392156863, -0.16462299647058826],
                      [-3.6588512862745097, 2.7129230470588235, 1.9459282392156863]])
BIAS = -0.0037930732552754493

BRADFORD = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])
BRADFORD_INV = np.array([[0.9869929, -0.1470543, 0.1599627], [0.4323053, 0.5183603, 0.0492912], [-0.0085287, 0.0400428, 0.9684867]])


def white_xyz(w):
    return np.array([w[0] / w[1], 1.0, (1 - w[0] - w[1]) / w[1]])


def primaries_to_xyz(p, w):
    """RGB -> XYZ of primaries p (rx, ry, gx, gy, bx, by) whose (1, 1, 1) is white w."""
    prim = np.array([[p[0], p[2], p[4]], [p[1], p[3], p[5]], [1 - p[0] - p[1], 1 - p[2] - p[3], 1 - p[4] - p[5]]])
    return prim @ np.diag(np.linalg.solve(prim, white_xyz(w)))


def adapt_to_d50(w):
    """Bradford adaptation of white w to D50 (the reference's D50 XYZ is 0.96422, 1, 0.82521)."""
    lms, lms50 = BRADFORD @ white_xyz(w), BRADFORD @ np.array([0.96422, 1.0, 0.82521])
    return BRADFORD_INV @ np.diag(lms50 / lms) @ BRADFORD


def srgb_to_target(p, w):
    """Linear sRGB -> linear RGB of primaries p, white w, through D50 XYZ (dec_xyb.cc:195-220)."""
    srgb_to_xyzd50 = adapt_to_d50(D65) @ primaries_to_xyz(SRGB, D65)
    return np.linalg.inv(adapt_to_d50(w) @ primaries_to_xyz(p, w)) @ srgb_to_xyzd50


def luminances(p, w):
    return primaries_to_xyz(p, w)[1]


def output_matrix(p, w, intensity_target=255.0, inv_opsin=INV_OPSIN):
    """The colour stage's matrix: XYB-mixed -> linear target RGB, 1.0 = the intensity target."""
    m = inv_opsin if (tuple(p) == SRGB and tuple(w) == D65) else srgb_to_target(p, w) @ inv_opsin
    return m * (255.0 / intensity_target)


def xyb_to_mixed(xyb):
    """xyb [3, n] -> the opsin-mixed values the matrix applies to (dec_xyb-inl.h:38-86)."""
    x, y, b = (np.asarray(c, np.float64) for c in xyb)
    cb = np.cbrt(BIAS)
    return np.stack([(y + x - cb) ** 3 + BIAS, (y - x - cb) ** 3 + BIAS, (b - cb) ** 3 + BIAS])


# ---- transfer functions (odd symmetry where the reference keeps the sign)
def srgb_encode(v):
    a = np.abs(v)
    return np.sign(v) * np.where(a <= 0.0031308, a * 12.92, 1.055 * np.power(np.maximum(a, 1e-30), 1 / 2.4) - 0.055)


PQ_M1, PQ_M2 = 2610 / 16384, 2523 / 4096 * 128
PQ_C1, PQ_C2, PQ_C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32


def pq_encode_nits(nits):
    """SMPTE ST 2084 inverse EOTF of luminance in cd/m2."""
    y = np.power(np.abs(nits) / 10000.0, PQ_M1)
    return np.copysign(np.power((PQ_C1 + PQ_C2 * y) / (1 + PQ_C3 * y), PQ_M2), nits)


def pq_decode_nits(e):
    p = np.power(np.abs(e), 1 / PQ_M2)
    return np.copysign(np.power(np.maximum(p - PQ_C1, 0) / (PQ_C2 - PQ_C3 * p), 1 / PQ_M1) * 10000.0, e)


HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073


def hlg_encode(v):
    a = np.abs(v)
    lo = np.sqrt(3 * a)
    hi = HLG_A * np.log(np.maximum(12 * a - HLG_B, 1e-30)) + HLG_C
    return np.copysign(np.where(a <= 1 / 12, lo, hi), v)


def rec709_encode(v):
    return np.where(v <= 0.018, 4.5 * v, 1.099 * np.power(np.maximum(v, 0.018), 0.45) - 0.099)


def gamma_encode(v, inv_gamma):
    return np.where(v <= 1e-5, 0.0, np.power(np.maximum(v, 1e-5), inv_gamma))


# ---- tone mapping
def hlg_ootf(rgb, exponent, lum):
    """HlgOOTF_Base::Apply on rgb [3, n]: times luminance^exponent, at most 1e9; pixels whose luminance is not positive
    stay as they are (the reference's power is undefined there)."""
    if -0.01 <= exponent <= 0.01:
        return rgb
    y = lum @ rgb
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(y > 0, np.minimum(np.power(np.where(y > 0, y, 1.0), exponent), 1e9), 1.0)
    return rgb * ratio


def hlg_to_scene_exponent(display_luminance):
    return (1 / 1.2) * 1.111 ** (-np.log2(display_luminance / 1000.0)) - 1


def hlg_tone_exponent(source, target):
    return 1.111 ** np.log2(target / source) - 1


def rec2408_tone_map(rgb, source_peak, target_peak, lum):
    """Rec2408ToneMapperBase::ToneMap with source range (0, source_peak), target range (0, target_peak)."""
    pq_min = pq_encode_nits(0.0)
    pq_range = pq_encode_nits(source_peak) - pq_min
    min_lum = (pq_encode_nits(0.0) - pq_min) / pq_range
    max_lum = (pq_encode_nits(target_peak) - pq_min) / pq_range
    ks = 1.5 * max_lum - 0.5
    y = source_peak * (lum @ rgb)
    npq = np.minimum(1.0, (pq_encode_nits(y) - pq_min) / pq_range)
    t = (npq - ks) / max(1e-6, 1 - ks)
    p = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
    e2 = np.where(npq < ks, npq, p)
    e3 = min_lum * (1 - e2) ** 4 + e2
    e4 = e3 * pq_range + pq_min
    new_y = np.clip(pq_decode_nits(e4), 0.0, target_peak)
    use_cap = y <= 1e-6
    ratio = new_y / np.maximum(y, 1e-6)
    return np.where(use_cap, new_y / target_peak, rgb * ratio * (source_peak / target_peak))


def gamut_map(rgb, lum, preserve_saturation=0.1):
    """GamutMapScalar on rgb [3, n]."""
    y = lum @ rgb
    sat = np.zeros_like(y)
    lumix = np.zeros_like(y)
    for c in range(3):
        v = rgb[c]
        d = v - y
        inv = 1.0 / np.where(d == 0, 1.0, d)
        over = v * inv
        sat = np.where(d >= 0, sat, np.maximum(sat, over))
        lumix = np.maximum(lumix, np.where(d <= 0, sat, over - inv))
    mix = np.clip(preserve_saturation * (sat - lumix) + lumix, 0.0, 1.0)
    out = mix * (y - rgb) + rgb
    return out / np.maximum(1.0, out.max(axis=0))


# ---- the whole stage
def render(linear, src_tf, intensity, dst_tf, desired=None, p=SRGB, w=D65, inv_gamma=None):
    """Linear RGB [3, n] in the target primaries (1.0 = the image's intensity target) -> the target encoding.
    src_tf / dst_tf: 'srgb', 'linear', 'pq', 'hlg', '709', 'gamma' (DCI: 'gamma' with inv_gamma 1 / 2.6)."""
    desired = intensity if desired is None else desired
    lum = luminances(p, w) if not (tuple(p) == SRGB and tuple(w) == D65) else np.array([0.2126, 0.7152, 0.0722])
    rgb = np.asarray(linear, np.float64)
    if desired != intensity:
        tone = None
        if src_tf == "pq" and desired < intensity:
            tone = "rec2408"
        elif src_tf == "hlg" and dst_tf != "hlg":
            tone = "hlg"
        if tone:
            pre, post = (10000.0 / intensity, desired / 10000.0) if dst_tf == "pq" else (1.0, 1.0)
            rgb = rgb * pre
            if tone == "rec2408":
                rgb = gamut_map(rec2408_tone_map(rgb, intensity, desired, lum), lum)
            else:
                e = hlg_tone_exponent(intensity, desired)
                rgb = hlg_ootf(rgb, e, lum)
                if (e < -0.01 or e > 0.01) and e < 0:
                    rgb = gamut_map(rgb, lum)
            rgb = rgb * post
    if dst_tf == "linear":
        return rgb
    if dst_tf == "srgb":
        return srgb_encode(rgb)
    if dst_tf == "pq":
        return pq_encode_nits(rgb * intensity)
    if dst_tf == "hlg":
        return hlg_encode(hlg_ootf(rgb, hlg_to_scene_exponent(desired), lum))
    if dst_tf == "709":
        return rec709_encode(rgb)
    if dst_tf == "gamma":
        return gamma_encode(rgb, inv_gamma)
    raise ValueError(dst_tf)
