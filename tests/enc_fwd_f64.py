"""A float64 NumPy reading of the forward VarDCT path (the encoder's pixel half: what jxlhip_enc_forward and the CPU stream
writer's model both produce as acs / qf / dc / coeffs), written from the reference's text and from this repository's
stated heuristics. It shares no code or tables with csrc/enc/jxl_enc.cc or the HIP kernels; the only inputs it takes from a
product are the quantiser fields of an encoded stream's headers, as the oracle decoder reads them.

The reference's parts:
  - sRGB8 -> linear: the exact sRGB EOTF in float64.
  - linear -> XYB: the opsin absorbance matrix and bias (lib/jxl/cms/opsin_params.h:36-60), cube root minus cbrt(bias),
    X = (L - M) / 2, Y = (L + M) / 2, B = S (enc_xyb.cc:50-104). The planes are padded to whole blocks by replicating the
    image's last column / row.
  - the forward DCT of every size class: the spec's scaled DCT-II (lib/jxl/dct_for_test.h:20-94, DCT1D: alpha(u) * cos *
    sqrt(2) / N), rows then columns, stored in the codestream layout: rows are the short side, and a transform with
    R >= C rows x columns is stored transposed ([kx][ky]).
  - DC: DCFromLowestFrequencies (enc_transforms-inl.h: ReinterpretingIDCT): the cy x cx lowest frequencies times
    DCTResampleScales<8n, n> (dct_scales.h), then the scaled cy x cx IDCT. The scales are computed here as the ratio
    of the lowest 8n-point DCT coefficients of a signal constant over 8-sample blocks to the n-point DCT coefficients of
    the block values, which reproduces the tables of dct_scales.h.
  - the Y dequantisation that chroma-from-luma predicts from: AdjustQuantBias with the default biases
    (quantizer.h:54, quantizer-inl.h:35-70; tests/golden/ref_constant_floats.json 'quant_bias'); X and B are residuals
    of x_cc * Y and b_cc * Y with the coded colour correlation (base 0 and 1, no per-tile factors: cfl_fit is not read).
  - the quantisation matrices: host_tables_np.compute_weights of the default library (pinned to the reference's text by
    test_host_tables.py); the quantiser multiplies X and B by 1.25 ** (x_qm_scale - 2) and 1.25 ** (b_qm_scale - 2)
    on top (enc_cache.cc:78-79, enc_group.cc:340-341), i.e. their steps are divided by it.

This repository's own choices (NOT the reference's: its encoder has an effort-dependent search instead):
  - sharpening: four rounds of y <- y + (x - K y) with K the decoder's normalised 3x3 Gaborish at the default weights
    (filters_f64.GAB_W1 / GAB_W2). Edge rule: a neighbour outside the PADDED plane is the nearest sample of the padded
    plane (clamped index; the padding samples take part in every round). The CPU writer (jxl_enc.cc:1976-1990) and all
    three kernel forms clamp to the padded plane (xp x yp); the kernels' "image coordinates" means plane coordinates as
    opposed to tile-local ones, not the unpadded image.
  - activity: the mean absolute deviation of Y from its mean per 8x8 block.
  - transform selection (strategy_mode 1): a greedy raster scan over the blocks; at each unassigned block the candidates
    64x64, 32x64, 64x32, 32x32, 16x32, 32x16, 16x16, 8x32, 32x8, 8x16, 16x8 are tried in that order, each taken if it is
    aligned to its own size, lies inside the frame and one 256x256 group, covers no assigned block, and the largest
    activity under it is below its threshold (d = distance): 0.004d, 0.0052d, 0.0052d, 0.008d, 0.011d, 0.011d, 0.016d,
    0.0128d, 0.0128d, 0.024d, 0.024d. Otherwise DCT8. strategy_mode 0: DCT8 everywhere.
  - quant field: mul = clamp(1.35 - 0.12 log2(1 + 400 m), 0.8, 1.4), m the largest activity under the transform,
    qf = clamp(floor(0.765 / d * mul * 65536 / global_scale + 0.5), 1, 256).
  - AC quantiser: v = coef / (m[k] * mulc), mulc = (65536 / global_scale) / qf * {x multiplier, 1, b multiplier};
    |v| < 0.58 -> 0, else v rounded to the nearest integer (ties to even). The reference's QuantizeBlockAC uses
    per-quadrant thresholds instead (enc_group.cc:336-364).
  - DC quantiser: round(dc / step), step = (65536 / global_scale) / quant_dc * dc_quant[c]; Y first, X and B as residuals
    of 0 * Y^ and 1 * Y^, Y^ the dequantised Y DC.

Layout of the outputs (what enc_forward_model returns): acs / qf [yb][xb]; dc [3][yb][xb]; coeffs [group][3][65536] with
group g = (by / 32) * xg + bx / 32 and the first blocks of a group in raster order, each taking R * C entries."""
import json
import os

import numpy as np

import host_tables_np as T
from filters_f64 import GAB_W1, GAB_W2

_GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_constant_floats.json")))

# opsin_params.h:36-60
_M00, _M02 = 0.30, 0.078
_M10, _M12 = 0.23, 0.078
_M20, _M21 = 0.24342268924547819, 0.20476744424496821
OPSIN = np.array([[_M00, 1.0 - _M02 - _M00, _M02], [_M10, 1.0 - _M12 - _M10, _M12], [_M20, _M21, 1.0 - _M20 - _M21]])
OPSIN_BIAS = float(_GOLDEN["opsin_bias"][0])
QUANT_BIAS = [float(v) for v in _GOLDEN["quant_bias"]]

# ac_strategy.h: blocks covered (x, y) and quantisation-table kind of the strategies the forward path selects
COVERED = {0: (1, 1), 4: (2, 2), 5: (4, 4), 6: (1, 2), 7: (2, 1), 8: (1, 4), 9: (4, 1), 10: (2, 4), 11: (4, 2),
           18: (8, 8), 19: (4, 8), 20: (8, 4)}
QUANT_KIND = {0: 0, 4: 4, 5: 5, 6: 6, 7: 6, 8: 7, 9: 7, 10: 8, 11: 8, 18: 11, 19: 12, 20: 12}
KINDS = sorted(COVERED)
# the selection scan's candidates in the order it tries them, with their thresholds in units of the distance
CANDIDATES = ((18, 0.004), (20, 0.004 * 1.3), (19, 0.004 * 1.3), (5, 0.008), (11, 0.011), (10, 0.011), (4, 0.016),
              (9, 0.016 * 0.8), (8, 0.016 * 0.8), (7, 0.016 * 1.5), (6, 0.016 * 1.5))
DEAD_ZONE = 0.58
K_AC_QUANT = 0.765


def srgb_to_linear(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def dct_matrix(n):
    """dct_for_test.h DCT1D: D[u, y] = alpha(u) cos((y + 1/2) u pi / n) sqrt(2) / n, alpha(0) = 1 / sqrt(2)."""
    u, y = np.mgrid[0:n, 0:n]
    a = np.where(u == 0, np.sqrt(0.5), 1.0)
    return a * np.cos((y + 0.5) * u * np.pi / n) * np.sqrt(2.0) / n


def idct_matrix(n):
    """The scaled IDCT the DC path applies (IDCT1D of dct_for_test.h divided by sqrt(n)): the inverse of dct_matrix."""
    return np.linalg.inv(dct_matrix(n))


def resample_scales(n):
    """DCTResampleScales<8n, n> (dct_scales.h), what DCFromLowestFrequencies multiplies the lowest frequencies by: per
    frequency i < n, the lowest 8n-point DCT coefficient of a signal that is constant over 8-sample blocks, divided by
    the n-point DCT coefficient of its block values (e.g. 0.901764195028874394 at <16, 2>). The decoder's
    LowestFrequenciesFromDC multiplies by the reciprocals (DCTResampleScales<n, 8n>)."""
    e = np.repeat(np.eye(n), 8, axis=0)  # [8n, n]: block values -> samples
    big = dct_matrix(8 * n)[:n] @ e      # [n, n]: each row a multiple of the same row of dct_matrix(n)
    small = dct_matrix(n)
    i = np.arange(n)
    return big[i, i] / small[i, i]


def opsin_xyb(img, xp, yp):
    """RGB8 [ys][xs][3] -> X, Y, B planes [3][yp][xp] (edge-replicated to whole blocks)."""
    ys, xs = img.shape[:2]
    lin = srgb_to_linear(np.asarray(img, np.float64) / 255.0)
    lin = np.pad(lin, ((0, yp - ys), (0, xp - xs), (0, 0)), mode="edge")
    mixed = lin @ OPSIN.T + OPSIN_BIAS
    g = np.cbrt(mixed) - np.cbrt(OPSIN_BIAS)
    return np.stack([0.5 * (g[..., 0] - g[..., 1]), 0.5 * (g[..., 0] + g[..., 1]), g[..., 2]])


def sharpen(planes, rounds=4):
    x = np.asarray(planes, np.float64)
    nrm = 1.0 / (1.0 + 4.0 * (GAB_W1 + GAB_W2))
    y = x.copy()
    _, h, w = x.shape
    for _ in range(rounds):
        p = np.pad(y, ((0, 0), (1, 1), (1, 1)), mode="edge")
        side = p[:, 1:h + 1, 0:w] + p[:, 1:h + 1, 2:w + 2] + p[:, 0:h, 1:w + 1] + p[:, 2:h + 2, 1:w + 1]
        corner = p[:, 0:h, 0:w] + p[:, 0:h, 2:w + 2] + p[:, 2:h + 2, 0:w] + p[:, 2:h + 2, 2:w + 2]
        y = y + (x - (y + GAB_W1 * side + GAB_W2 * corner) * nrm)
    return y


def quantise_ac(v):
    """The repo's AC quantiser: dead zone |v| < 0.58, otherwise nearest integer, ties to even (monotone in v)."""
    v = np.asarray(v, np.float64)
    return np.where(np.abs(v) < DEAD_ZONE, 0, np.rint(v)).astype(np.int64)


def round_dc(v):
    """lround: nearest integer, ties away from zero."""
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def quant_field_int(t):
    return np.clip(np.floor(np.asarray(t, np.float64)), 1, 256).astype(np.int64)


def y_dequant_bias(q):
    """AdjustQuantBias for channel 1 (Y): 0, +-biases[1], or q - biases[3] / q."""
    q = np.asarray(q, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        far = q - QUANT_BIAS[3] / q
    return np.where(q == 0, 0.0, np.where(np.abs(q) == 1, np.sign(q) * QUANT_BIAS[1], far))


def header_scalars(J, distance):
    """The quantiser fields of the headers of the CPU writer's stream at `distance`, as the oracle decoder reads them.
    (These fields depend on the distance alone; a 64x64 frame is used so that the stream is cheap and has DC groups.)"""
    import jxlo
    img = J.synth_image(64, 64, seed=5)
    data = J.encode_rgb8(img, distance=distance)
    o = jxlo.Decoded(data, dumps=False)
    h = o.quant_header
    o.close()
    return h


class Reading:
    """The reading of one frame. Construction does the pixel stages, the activity and the reading's own transform
    selection; quant_field() / transform() take the transform choices (and the integer decisions the later stages build
    on) as arguments, so that each stage is judged given the decisions before it."""

    def __init__(self, img, header, distance=1.0, gab=1, strategy_mode=1):
        img = np.asarray(img, np.uint8)
        self.ys, self.xs = img.shape[:2]
        self.xb, self.yb = (self.xs + 7) // 8, (self.ys + 7) // 8
        self.xg, self.yg = (self.xs + 255) // 256, (self.ys + 255) // 256
        self.distance, self.strategy_mode = float(distance), int(strategy_mode)
        self.h = header
        gs = float(header["global_scale"])
        self.inv_gs = 65536.0 / gs
        self.dc_step = np.array([self.inv_gs / header["quant_dc"] * q for q in header["dc_quant"]])
        # (enc_cache.cc:78-79 multiplies the inverse matrix, which the quantiser multiplies by: the step is divided)
        self.cmul = np.array([1.25 ** (2 - header["x_qm_scale"]), 1.0, 1.25 ** (2 - header["b_qm_scale"])])
        self.cc = (header["base_corr_x"], header["base_corr_b"])
        xyb = opsin_xyb(img, self.xb * 8, self.yb * 8)
        self.planes = sharpen(xyb) if gab else xyb
        yb, xb = self.yb, self.xb
        blocks = self.planes[1].reshape(yb, 8, xb, 8)
        self.act = np.abs(blocks - blocks.mean(axis=(1, 3), keepdims=True)).mean(axis=(1, 3))
        self.acs, self.act_margin = self._select()

    # ---------------------------------------------------------------- selection
    def _select(self):
        """Greedy raster scan, vectorised over the 64x64 tiles (every candidate is aligned to its own size, so the scan
        never looks outside the tile). Returns acs and, per tile, the smallest |region max - threshold| of the
        activity tests the scan consulted there (infinite where it consulted none)."""
        yb, xb = self.yb, self.xb
        ty, tx = (yb + 7) // 8, (xb + 7) // 8
        a = np.full((ty * 8, tx * 8), np.inf)
        a[:yb, :xb] = self.act
        tiles = a.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 8, 8)
        nt = tiles.shape[0]
        st = np.zeros((nt, 8, 8), np.int64)
        first = np.zeros((nt, 8, 8), bool)
        margin = np.full(nt, np.inf)
        if self.strategy_mode == 1:
            rmax, thr = {}, {}
            for s, t in CANDIDATES:
                cx, cy = COVERED[s]
                rmax[s] = tiles.reshape(nt, 8 // cy, cy, 8 // cx, cx).max(axis=(2, 4))
                thr[s] = t * self.distance
            occupied = np.zeros((nt, 8, 8), bool)
            for by in range(8):
                for bx in range(8):
                    todo = ~occupied[:, by, bx]
                    for s, _ in CANDIDATES:
                        cx, cy = COVERED[s]
                        if by % cy or bx % cx or by + cy > 8 or bx + cx > 8:
                            continue
                        r = rmax[s][:, by // cy, bx // cx]
                        fits = todo & np.isfinite(r) & ~occupied[:, by:by + cy, bx:bx + cx].any(axis=(1, 2))
                        margin = np.where(fits, np.minimum(margin, np.abs(r - thr[s])), margin)
                        take = fits & (r < thr[s])
                        st[take, by:by + cy, bx:bx + cx] = s
                        occupied[take, by:by + cy, bx:bx + cx] = True
                        first[take, by, bx] = True
                        todo &= ~take
                    first[todo, by, bx] = True
                    occupied[todo, by, bx] = True
        else:
            first[:] = True
        acs = ((st << 1) | first).astype(np.uint8)
        acs = acs.reshape(ty, tx, 8, 8).transpose(0, 2, 1, 3).reshape(ty * 8, tx * 8)[:yb, :xb]
        return acs, margin.reshape(ty, tx)

    # ---------------------------------------------------------------- quant field
    def _region_max(self, acs):
        """Per first block: the largest activity under its transform (0 elsewhere)."""
        m = np.zeros((self.yb, self.xb))
        for s, (by, bx) in self._firsts(acs):
            cx, cy = COVERED[s]
            r = self.act[by[:, None, None] + np.arange(cy)[None, :, None], bx[:, None, None] + np.arange(cx)[None, None, :]]
            m[by, bx] = r.max(axis=(1, 2))
        return m

    def quant_field(self, acs):
        """The value before rounding, t = 0.765 / d * mul * 65536 / global_scale + 0.5, at first blocks of `acs`
        (qf = quant_field_int(t)); NaN elsewhere."""
        m = self._region_max(acs)
        mul = np.clip(1.35 - 0.12 * np.log2(1.0 + m * 400.0), 0.8, 1.4)
        t = K_AC_QUANT / self.distance * mul * self.inv_gs + 0.5
        return np.where(acs & 1, t, np.nan)

    # ---------------------------------------------------------------- transforms
    @staticmethod
    def _firsts(acs):
        out = []
        for s in KINDS:
            by, bx = np.nonzero(acs == ((s << 1) | 1))
            if len(by):
                out.append((s, (by, bx)))
        return out

    def layout(self, acs):
        """Per strategy: the (group, offset) of each of its first blocks in the [group][3][65536] arrays."""
        by, bx = np.nonzero(acs & 1)  # raster order
        st = acs[by, bx] >> 1
        size = np.array([64 * COVERED[int(s)][0] * COVERED[int(s)][1] for s in st])
        g = (by // 32) * self.xg + bx // 32
        order = np.lexsort((bx, by, g))  # by group, raster inside the group
        off = np.zeros(len(by), np.int64)
        gs, sz = g[order], size[order]
        csum = np.cumsum(sz) - sz
        start = np.zeros(len(gs), np.int64)
        newg = np.r_[True, gs[1:] != gs[:-1]]
        start[newg] = csum[newg]
        start = np.maximum.accumulate(start)
        off[order] = csum - start
        where = {}
        for s in np.unique(st):
            sel = st == s
            where[int(s)] = (by[sel], bx[sel], g[sel], off[sel])
        return where

    def coefficients(self, acs):
        """Per strategy s: natural-layout float64 coefficients [3][n][R][C] of its transforms (first blocks in raster)."""
        out = {}
        for s, (by, bx) in self._firsts(acs):
            cx, cy = COVERED[s]
            R, C = 8 * cy, 8 * cx
            rows = by[:, None] * 8 + np.arange(R)[None]
            cols = bx[:, None] * 8 + np.arange(C)[None]
            px = self.planes[:, rows[:, :, None], cols[:, None, :]]  # [3][n][R][C]
            out[s] = np.einsum("ur,cnrx,vx->cnuv", dct_matrix(R), px, dct_matrix(C), optimize=True)
        return out

    def transform(self, acs, qf, dc_y=None, coeffs_y=None):
        """Values before rounding of the DC and AC integers, given the transform choices `acs`, the quant field `qf` and
        optionally the Y integers (DC [yb][xb], coeffs [group][65536]) the chroma-from-luma residuals are formed against
        (default: the reading's own rounding of Y). Returns (dc [3][yb][xb], coeffs [group][3][65536], mask of the
        coefficient positions that carry a value)."""
        yb, xb, ng = self.yb, self.xb, self.xg * self.yg
        dc = np.zeros((3, yb, xb))
        co = np.zeros((ng, 3, 65536))
        used = np.zeros((ng, 65536), bool)
        coefs = self.coefficients(acs)
        where = self.layout(acs)
        weights = {}
        for s, nat in coefs.items():
            cx, cy = COVERED[s]
            R, C = 8 * cy, 8 * cx
            by, bx, g, off = where[s]
            n = len(by)
            # DC: lowest frequencies x resample scales, scaled IDCT of cy x cx, per covered block
            llf = nat[:, :, :cy, :cx] * resample_scales(cy)[None, None, :, None] * resample_scales(cx)[None, None, None, :]
            blk = np.einsum("yu,cnuv,xv->cnyx", idct_matrix(cy), llf, idct_matrix(cx))
            ry = by[:, None, None] + np.arange(cy)[None, :, None] + 0 * np.arange(cx)[None, None, :]
            rx = bx[:, None, None] + np.arange(cx)[None, None, :] + 0 * np.arange(cy)[None, :, None]
            vy = blk[1] / self.dc_step[1]
            qy = round_dc(vy) if dc_y is None else dc_y[ry, rx]
            yhat = qy * self.dc_step[1]
            dc[1, ry, rx] = vy
            dc[0, ry, rx] = (blk[0] - self.cc[0] * yhat) / self.dc_step[0]
            dc[2, ry, rx] = (blk[2] - self.cc[1] * yhat) / self.dc_step[2]
            # AC: codestream layout (rows = short side, transposed when R >= C)
            stored = nat if R < C else nat.transpose(0, 1, 3, 2)
            stored = stored.reshape(3, n, R * C)
            kind = QUANT_KIND[s]
            if kind not in weights:
                weights[kind] = 1.0 / T.compute_weights(kind, T.library_encoding(kind, _GOLDEN["quant_library"])).astype(np.float64)
            m = weights[kind].reshape(3, 1, R * C)
            lrows, lcols = min(cx, cy), max(cx, cy)
            k = np.arange(R * C)
            ac = ~((k // (8 * lcols) < lrows) & (k % (8 * lcols) < lcols))
            scaled = self.inv_gs / qf[by, bx].astype(np.float64)
            step = m * (scaled[None, :, None] * self.cmul[:, None, None])  # [3][n][RC]
            idx = off[:, None] + k[None]
            vyac = stored[1] / step[1]
            qyac = quantise_ac(vyac) if coeffs_y is None else coeffs_y[g[:, None], idx]
            ydeq = y_dequant_bias(qyac) * step[1]
            vals = np.stack([(stored[0] - self.cc[0] * ydeq) / step[0], vyac, (stored[2] - self.cc[1] * ydeq) / step[2]])
            vals = np.where(ac[None, None], vals, 0.0)
            for c in range(3):
                co[g[:, None], c, idx] = vals[c]
            used[g[:, None], idx] = ac[None]
        return dc, co, used


def decide(got, value, f, delta):
    """The one comparison rule of the forward path against this reading. `value` is the float64 reading of a quantity
    before the monotone rounding `f` turns it into the integer the product emitted (`got`); `delta` bounds the error of
    the product's float32 chain in the units of `value`. Where f(value - delta) == f(value + delta) no float32 evaluation
    can land on another integer, and `got` must equal it exactly; otherwise the value lies within delta of a decision
    boundary (a half-integer, the +-0.58 dead zone, the quant field's integer after +0.5) and either neighbour is
    accepted. Returns (mask of the ambiguous values, mask of the wrong ones).

    DELTA, per quantity, in the units of `value` (DC and AC: their quantisation steps; qf: the quant field before
    truncation; act: the activity, which the selection compares with the thresholds). It was measured on the CPU
    writer's model, whose float32 chain (cube root, four sharpening rounds, DCT sums of up to 64 terms per pass) the
    kernels restate: with delta = 0, over the cases of test_enc_fwd_f64.py (sizes 8x8 .. 1000x700, distances 0.3 / 1 / 4,
    gab 0 / 1, strategy modes 0 / 1, the mosaic), every DC and AC integer the model rounded differently from the
    reading lay within DELTA_MEASURED of the boundary (DC 1.12e-5 steps, AC 1.08e-5 steps); DELTA is about four
    times that. The quant field and the transform choices never differed; their delta is the float32 error bound of
    the value (t ~ 100: 1e-4; the activity, a mean of 64 deviations of samples that carry errors of a few float32 ulps of
    ~0.5: 3e-7)."""
    value = np.asarray(value, np.float64)
    lo, hi = f(value - delta), f(value + delta)
    got = np.asarray(got).astype(np.int64)
    return lo != hi, (got < lo) | (got > hi)


DELTA_MEASURED = {"dc": 1.12e-5, "ac": 1.08e-5}
DELTA = {"act": 3e-7, "qf": 1e-4, "dc": 5e-5, "ac": 5e-5}


def check_forward(model, img, header, distance=1.0, gab=1, strategy_mode=1, max_band=1e-3):
    """Holds one output of enc_forward_model to the reading: transform choices exactly outside 64x64 tiles whose scan
    consulted an activity within DELTA['act'] of a threshold (at most 1 % of the tiles, or one tile), then the quant
    field, the DC and the AC integers under the model's own transform choices, each by decide();
    the ambiguous band of each must hold less than `max_band` of the compared values. Returns the sizes of the bands."""
    R = Reading(img, header, distance=distance, gab=gab, strategy_mode=strategy_mode)
    acs = model["acs"]
    assert acs.shape == R.acs.shape
    ty, tx = R.act_margin.shape
    amb_tiles = np.repeat(np.repeat(R.act_margin <= DELTA["act"], 8, 0), 8, 1)[:R.yb, :R.xb]
    bad = (acs != R.acs) & ~amb_tiles
    assert not bad.any(), "transform choice differs from the reading at %d blocks, first (by, bx) %s: %d, reading %d" % (
        bad.sum(), tuple(np.argwhere(bad)[0]), acs[bad][0], R.acs[bad][0])
    n_amb_tiles = int((R.act_margin <= DELTA["act"]).sum())
    assert n_amb_tiles <= max(1, 0.01 * ty * tx), n_amb_tiles
    first = (acs & 1) == 1
    t = R.quant_field(acs)
    amb_q, wrong = decide(model["qf"][first], t[first], quant_field_int, DELTA["qf"])
    assert not wrong.any(), "quant field differs at %d first blocks: %s vs reading %s" % (
        wrong.sum(), model["qf"][first][wrong][:4], t[first][wrong][:4])
    dc, co, used = R.transform(acs, model["qf"], dc_y=model["dc"][1], coeffs_y=model["coeffs"][:, 1])
    amb_d, wrong = decide(model["dc"], dc, round_dc, DELTA["dc"])
    assert not wrong.any(), "DC differs at %d of %d (channel, by, bx) %s: %d vs reading %.4f" % (
        wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]), model["dc"][wrong][0], dc[wrong][0])
    sel = np.broadcast_to(used[:, None, :], co.shape)
    amb_a, wrong = decide(model["coeffs"][sel], co[sel], quantise_ac, DELTA["ac"])
    if wrong.any():
        g, c, k = np.argwhere(sel)[np.flatnonzero(wrong)[0]]
        raise AssertionError("AC differs at %d of %d, first group %d channel %d index %d: %d vs reading %.4f" % (
            wrong.sum(), wrong.size, g, c, k, model["coeffs"][g, c, k], co[g, c, k]))
    bands = {"tiles": n_amb_tiles, "qf": int(amb_q.sum()), "dc": int(amb_d.sum()), "ac": int(amb_a.sum()),
             "n_qf": int(first.sum()), "n_dc": int(dc.size), "n_ac": int(sel.sum())}
    for k in ("qf", "dc", "ac"):
        assert bands[k] <= max_band * bands["n_" + k], bands
    return bands


def mosaic(xs=685, ys=419, amp=0.5, seed=3):
    """An image whose 64x64 tiles each hold one smooth region of a designed shape among textured 8x8 blocks, so that the
    greedy scan places every size class: the smooth region of tile t is the footprint of size class
    MOSAIC_SHAPES[t % 11] at the tile's top-left (or, every other pass through the list, at its far corner where the
    shape allows), and the rest of the tile is high-contrast noise (which keeps DCT8). The smooth content is a gentle
    two-dimensional cosine whose activity stays below every threshold at distance 1 without sharpening (amp scales it), whose
    large transforms still carry non-zero AC. The default size has ragged right and bottom edges (xb = 86, yb = 53) and
    group boundaries every 4 tiles."""
    rng = np.random.default_rng(seed)
    xb, yb = (xs + 7) // 8, (ys + 7) // 8
    smooth = np.zeros((yb, xb), bool)
    tx, ty = (xb + 7) // 8, (yb + 7) // 8
    for t in range(tx * ty):
        cx, cy = COVERED[MOSAIC_SHAPES[t % 11]]
        by0, bx0 = (t // tx) * 8, (t % tx) * 8
        if (t // 11) % 2:
            by0, bx0 = by0 + 8 - cy, bx0 + 8 - cx
        smooth[by0:by0 + cy, bx0:bx0 + cx] = True
    yy, xx = np.mgrid[0:yb * 8, 0:xb * 8]
    soft = 120 + amp * (14 * np.cos(xx * np.pi / 61.0) + 10 * np.cos(yy * np.pi / 47.0 + 1.0))
    noise = rng.integers(30, 226, (yb * 8, xb * 8))
    grey = np.where(np.repeat(np.repeat(smooth, 8, 0), 8, 1), soft, noise)
    img = np.stack([grey, grey * 0.9 + 12, grey * 0.8 + 30], axis=-1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)[:ys, :xs]


MOSAIC_SHAPES = (18, 20, 19, 5, 11, 10, 4, 9, 8, 7, 6)
