"""A float64 NumPy reading of the reference's initial adaptive quant field, written from the text of
lib/jxl/enc_adaptive_quantization.cc (line numbers below are that file's unless another is named) and sharing no code
with csrc/enc/jxl_enc.cc or the HIP kernels. It may borrow XYB, the transform choices and decide() from enc_fwd_f64.

What the encoder's adaptive_quant=1 mode states (and this reading restates in float64, whole-array):

  input     the X, Y, B planes padded to whole blocks, BEFORE the sharpening (enc_heuristics.cc:1118-1143); a neighbour
            outside the padded plane is the nearest sample of the padded plane (x1 / x2 / y1 / y2 of :502-510).
            d_iqf = d with Gaborish, 0.62 d without (enc_heuristics.cc:1119-1122); scale = 0.765 / d_iqf * rescale (:1268).
  cells     ComputeTile :528-611. Per pixel base = 0.25 (down + up + left + right), g = ratio<false>(Y + 0.019),
            v = min((g (Y - base))^2, 0.2), p = MaskingSqrt(v) = 0.25 sqrt(v sqrt(211.66567973503678e8) + 27.505837037000106)
            (:351-357). A cell is one per 4x4 pixels: the SUM over its four rows of p, averaged over its four columns.
  ratio     RatioOfDerivativesOfCubicRootToSimpleGamma :127-145, v clamped at 0: num = kNumMul v^2 + eps,
            den = kDenMul v^3 + kVOffset; <false> is den / num, <true> num / den.
  erosion   FuzzyErosion :389-449: per cell the four smallest of its 3x3 neighbourhood (clamped at the borders of the cell
            image) weighted by kMul[0..3] (kMulBase + mul kMulAdd, mul = (2 - d_iqf) / 2 below 2, normalised to kTotal);
            a block's e is the sum over its 2x2 cells. The reference's 64x64 tiles carry one border cell of their
            neighbours (:534-537, from_rect :614): one global cell image, no seam.
  mask      1 / (e + 0.001) (:88-92).
  field     PerBlockModulations :315-348: m = ComputeMask(e) (:95-117); m += 0.1005613337192697 log2(mean over the 64
            pixels of (ratio<true>(Y + 0.16 - X) + ratio<true>(Y + 0.16 + X)) / 2) (:179-211);
            hf = m + 0.42 - 0.38 sum min(0.0206, |dY|) over the 7 horizontal pairs of each row and the 8 vertical pairs of
            each column with row 7 paired with itself (:260-313); blue = m + BlueModulation (:221-256, both folds);
            aq = 2^(min(hf, blue) 1.442695041) mul + add with the dampen ramp of :319-331.
  aggregate AdjustQuantField :1198-1247 with the frame's own d: the max over a transform's blocks, mixed with their mean
            by mean_max_mixer from four blocks on; integer field = clamp(trunc(value 65536 / global_scale + 0.5), 1, 256)
            (quantizer.cc:78-88, quantizer.h:68-71).
  scalars   global_scale / quant_dc from ComputeGlobalScaleAndQuant(InitialQuantDC(d), 0.39 / d, 0)
            (enc_heuristics.cc:1128-1129, quantizer.cc:45-76).
Deviation from the reference shared with the product: log2 / 2^x are exact here and in the product (log2f / exp2f), where
the reference has FastLog2f / FastPow2f (relative error 3e-7, base/fast_math-inl.h:46,70).

Measured margins (the CPU double / the CPU model against this reading; test_adaptive_quant_f64.py prints them with -s):
  RTOL_MEASURED  the largest relative deviation |product - reading| / |reading| of aq_map and mask over exactly the cases
                 of test_adaptive_quant_f64.py (6 plane kinds x 7 sizes x 6 distances); RTOL is four times that.
  QF_DELTA_MEASURED  over the whole-path cases, the largest distance from the truncation boundary (in units of the value
                 before truncation, t = value 65536 / global_scale + 0.5) among the integers the CPU model rounded
                 differently from the reading. No integer differed (14814 first blocks, t = 1.5 .. 17), so four times the
                 measurement is no bound; as enc_fwd_f64.decide does for its quant field, delta is then the float32 error
                 bound of the value: the field's relative bound RTOL (measured from float32 planes on) and as much again
                 for the float32 planes themselves (cbrtf and the opsin sums: a few 1e-8 on Y, which the Laplacian of the
                 cells turns into about 2e-6 of a cell at the contrasts where it is steepest), times t:
                 delta = QF_DELTA_REL t with QF_DELTA_REL = 2 RTOL."""
import numpy as np

K_INV_LOG2E = 0.6931471805599453
K_SG_MUL = 226.77216153508914
K_SG_MUL2 = 1.0 / 73.377132366608819
K_SG_RET_MUL = K_SG_MUL2 * 18.6580932135 * K_INV_LOG2E
K_SG_V_OFFSET = 7.7825991679894591
K_AC_QUANT = 0.765

RTOL_MEASURED = 2.13e-6  # (mask, the negative plane at 264x264 d 0.3; aq_map: 1.02e-6, the ramps at 264x264 d 1.9)
RTOL = 4 * RTOL_MEASURED
QF_DELTA_MEASURED = 0.0
QF_DELTA_REL = 2 * RTOL


def ratio(v, invert):
    eps = 1e-2
    v = np.maximum(np.asarray(v, np.float64), 0.0)
    num = K_SG_RET_MUL * 3 * K_SG_MUL * v * v + eps
    den = K_INV_LOG2E * K_SG_MUL * v * v * v + (K_SG_V_OFFSET * K_INV_LOG2E + eps)
    return num / den if invert else den / num


def masking_sqrt(v):
    return 0.25 * np.sqrt(v * np.sqrt(211.66567973503678 * 1e8) + 27.505837037000106)


def cell_image(y):
    """[yp][xp] -> [yp / 4][xp / 4]"""
    y = np.asarray(y, np.float64)
    h, w = y.shape
    p = np.pad(y, 1, mode="edge")
    base = 0.25 * (p[2:, 1:-1] + p[:-2, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:])
    v = np.minimum((ratio(y + 0.019, False) * (y - base)) ** 2, 0.2)
    return masking_sqrt(v).reshape(h // 4, 4, w // 4, 4).sum(axis=1).mean(axis=2)


def erosion_weights(d_iqf):
    base = np.array([0.125, 0.1, 0.09, 0.06])
    add = np.array([0.0, -0.1, -0.09, -0.06])
    mul = (2.0 - d_iqf) * 0.5 if d_iqf < 2.0 else 0.0
    k = base + mul * add
    return k * (0.29959705784054957 / k.sum())


def fuzzy_erosion(cells, d_iqf):
    """[ch][cw] -> e [ch / 2][cw / 2]"""
    ch, cw = cells.shape
    p = np.pad(cells, 1, mode="edge")
    nine = np.stack([p[dy:dy + ch, dx:dx + cw] for dy in range(3) for dx in range(3)])
    four = np.sort(nine, axis=0)[:4]
    v = np.tensordot(erosion_weights(d_iqf), four, axes=1)
    return v.reshape(ch // 2, 2, cw // 2, 2).sum(axis=(1, 3))


def compute_mask(e):
    v1 = np.maximum(e * 0.80061762862741759, 1e-3)
    off3 = 3.7179635626140772
    v2 = 1.0 / (v1 + 302.59587815579727)
    v3 = 1.0 / (v1 * v1 + off3)
    v4 = 1.0 / (v1 * v1 + 0.25 * off3)
    return -0.7647 + 9.4708735624378946 * v4 + 17.35036561631863 * v2 + 6.7943250517376494 * v3


def _blocks(a):
    h, w = a.shape
    return a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [yb][xb][8][8]


def gamma_modulation(x, y):
    bx, by = _blocks(x), _blocks(y) + 0.16
    overall = (ratio(by - bx, True) + ratio(by + bx, True)).sum(axis=(2, 3)) * (0.5 / 64)
    return 0.1005613337192697 * np.log2(overall)


def hf_modulation(y):
    b = _blocks(y)
    lim = 0.0206
    s = np.minimum(lim, np.abs(b[..., :, :-1] - b[..., :, 1:])).sum(axis=(2, 3))
    s = s + np.minimum(lim, np.abs(b[..., :-1, :] - b[..., 1:, :])).sum(axis=(2, 3))  # (row 7 against itself adds 0)
    return s * -0.38 + 0.42


def blue_modulation(x, y, b):
    lim, off, kmax = 0.010474084867598155, 0.0031994768654636393, 15.463398341612438
    eff = _blocks(y) + off + np.abs(_blocks(x))
    bb = _blocks(b)
    s = np.where(bb > eff, np.minimum(bb - eff, lim), 0.0).sum(axis=(2, 3))
    s = np.where(s >= 32 * lim, 64 * lim - s, s)
    s = np.where(s >= kmax * lim, kmax * lim, s)
    return s * 0.90590804735610064


def dampen(d_iqf):
    if d_iqf < 2.0:
        return 1.0
    return max(0.0, 1.0 - (d_iqf - 2.0) / (14.0 - 2.0))


def initial_quant_field(xyb, d_iqf, rescale=1.0):
    """X, Y, B planes [3][yp][xp] (multiples of 8) -> (aq_map, mask), both [yp / 8][xp / 8], float64."""
    x, y, b = (np.asarray(p, np.float64) for p in xyb)
    e = fuzzy_erosion(cell_image(y), d_iqf)
    mask = 1.0 / (e + 0.001)
    m = compute_mask(e) + gamma_modulation(x, y)
    out = np.minimum(m + hf_modulation(y), m + blue_modulation(x, y, b))
    scale = K_AC_QUANT / d_iqf * rescale
    dmp = dampen(d_iqf)
    return np.exp2(out * 1.442695041) * (scale * dmp) + (1.0 - dmp) * (0.48 * scale), mask


def mean_max_mixer(distance):
    if distance <= 1.54138:
        return 1.0
    return max(0.0, 1.0 - (distance - 1.54138) * 0.56391)


def adjust_quant_field(aq, acs, distance, covered):
    """AdjustQuantField: the field's value at the first blocks of `acs` (NaN elsewhere). covered: strategy -> (cx, cy)."""
    mix = mean_max_mixer(distance)
    out = np.full(aq.shape, np.nan)
    for s, (cx, cy) in covered.items():
        by, bx = np.nonzero(acs == ((s << 1) | 1))
        if not len(by):
            continue
        r = aq[by[:, None, None] + np.arange(cy)[None, :, None], bx[:, None, None] + np.arange(cx)[None, None, :]]
        mx, mean = r.max(axis=(1, 2)), r.mean(axis=(1, 2))
        out[by, bx] = mx * mix + (1.0 - mix) * mean if cx * cy >= 4 else mx
    return out


def quantizer_scalars(distance):
    """(global_scale, quant_dc) of ComputeGlobalScaleAndQuant(InitialQuantDC(d), 0.39 / d, 0)."""
    target_dc = max(0.5 * distance, min(distance, 0.3 * (distance / 0.3) ** 0.83))
    qdc = min(1.095924047623553 / target_dc, 50.0)
    scale = min(max(65536.0 * (0.39 / distance) / 5.0, 1.0), 32768.0)
    gs = int(scale)
    scaled = int(qdc * 4096 * 1.6)
    if gs > scaled:
        gs = max(scaled, 1)
    return gs, int(min(65536.0, qdc * (65536.0 / gs) + 0.5))


# ---------------------------------------------------------------- the crafted planes of the stand-alone entry's tests
SIZES = ((8, 8), (16, 8), (8, 16), (72, 72), (136, 72), (104, 24), (264, 264))  # (xsize, ysize)
DISTANCES = (0.3, 1.0, 1.9, 2.5, 4.0, 15.0)
KINDS = ("ramps", "flat", "noise", "blue", "negative", "steps")


def crafted(kind, xs, ys, seed=7):
    """X, Y, B planes [3][ys][xs], float32 (what both the product and the reading are given)."""
    rng = np.random.default_rng(seed + 131 * xs + ys)
    yy, xx = np.mgrid[0:ys, 0:xs].astype(np.float64)
    if kind == "ramps":
        x = 0.02 * np.sin(xx / 23.0) + 0.0004 * yy
        y = 0.05 + 0.6 * xx / max(xs, 64) + 0.2 * yy / max(ys, 64)
        b = y + 0.1 * np.cos(yy / 17.0)
    elif kind == "flat":
        x, y, b = np.full((ys, xs), 0.01), np.full((ys, xs), 0.4), np.full((ys, xs), 0.35)
    elif kind == "noise":
        x = 0.03 * rng.uniform(-1, 1, (ys, xs))
        y = 0.45 + 0.3 * rng.uniform(-1, 1, (ys, xs))
        b = 0.45 + 0.3 * rng.uniform(-1, 1, (ys, xs))
    elif kind == "blue":
        # the share of a block's pixels whose B lies far above Y + |X| runs from none to all along x (and y on narrow
        # planes): sums below kMaxLimit, between it and 32 kLimit (capped), and beyond 32 kLimit (folded, then capped or not)
        x = 0.01 * np.sin(xx / 5.0 + yy / 7.0)
        y = 0.25 + 0.1 * xx / max(xs, 64)
        share = ((xx // 8) * 8 / max(xs - 8, 1) + (yy // 8) * 8 / max(ys - 8, 1)) / (2.0 if xs > 8 and ys > 8 else 1.0)
        far = rng.uniform(0, 1, (ys, xs)) < share
        b = np.where(far, y + 0.5, y + np.abs(x) + 0.004 * rng.uniform(0, 1, (ys, xs)))
    elif kind == "negative":
        x = 0.05 * np.cos(xx / 3.0)
        y = -0.3 + 0.45 * (xx + yy) / (xs + ys) + 0.02 * rng.uniform(-1, 1, (ys, xs))
        b = y + 0.05
    elif kind == "steps":
        x = np.zeros((ys, xs))
        y = np.where(((xx // 3) + (yy // 2)) % 2 == 0, 0.1, 0.9) + 0.01 * rng.uniform(-1, 1, (ys, xs))
        b = y.copy()
    else:
        raise ValueError(kind)
    return np.stack([x, y, b]).astype(np.float32)
