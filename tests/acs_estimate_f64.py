"""A float64 NumPy reading of the cost estimate of the reference's AC-strategy search, EstimateEntropy
(lib/jxl/enc_ac_strategy.cc:364-511; line numbers below are that file's) with the weights of AcStrategyHeuristics::Init
(:1107-1123), for the pure-DCT transforms up to 64x64. It shares no code with csrc/enc/jxl_enc.cc, the HIP kernels or the
oracle; it borrows other readings: the DCT matrices of enc_fwd_f64, the dequantisation weights of host_tables_np and the
crafted planes of adaptive_quant_f64.

  inputs        the X, Y, B planes, the quant field per block (config.Quant: the initial adaptive quant field), mask1x1 per
                pixel, one chroma-from-luma factor pair per 64x64 tile, the distance, and per candidate the transform, its
                top-left block and the multiplier entropy_mul.
  transform     TransformFromPixels :375-379: the scaled DCT of enc_fwd_f64.dct_matrix on rows and columns. The reference
                keeps the coefficients of a transform with R >= C rows x columns transposed ([kx][ky]); its weight tables
                (config.dequant->Matrix / InvMatrix, :422-423) are in that layout too. The reading keeps everything in
                the natural layout [ky][kx] and transposes the weights instead.
  quant_norm16  :384-414: one block: the block's field value; two: the larger of the two; four or more: the mean of the
                16th powers, to the power 1 / 16 (FastPowf in the reference; the exact power here and in the product).
  val           :428-432, over EVERY coefficient (the lowest frequencies too):
                val = (coef_c - coef_Y * cmap_c) * (inv_matrix * quant_norm16), cmap = {YtoXRatio, 0, YtoBRatio} of the
                tile (ProcessRectACS :850-854; chroma_from_luma.h:51-57: base + v / 84, base 0 for X and 1 for B).
  bits          :433-443, 488-495: per channel cost_delta * sum sqrt(|round(val)|) + zeros_mul * (CeilLog2(nbits + 17) + nbits),
                nbits = CeilLog2(nz + 1) + 1, nz the number of non-zero roundings. Round is to nearest, ties to even.
  loss          :436, 446-487: matrix * (val - round(val)) taken back to pixels (TransformToPixels), times
                mask1x1 + {12, 0, 4}, to the eighth power, summed, times {8.2, 1, 1.03} ** 8.
  X's weight    :496-502: entropy is a RUNNING sum over X, Y, B; after channel 0, for two blocks or more, it and the loss
                so far (X's shares alone) are multiplied by w = 1 + min(3, num_blocks / 8).
  result        :504-509: pow(loss / area, 1 / 8) * area / quant_norm16; entropy * entropy_mul + info_loss_multiplier * that.
  weights       :1111-1123: info_loss_multiplier 1.2, zeros_mul 9.3089059022677905, cost_delta 10.833273317067883, times
                ((distance + kBias) / (1 + kBias)) ** {kPow1, kPow2, kPow3}.

estimate() takes the roundings as an argument, so that the estimate can be evaluated under the product's own round(val):
what is left then is continuous in the inputs. MISREADINGS are deliberate wrong readings of the above;
test_acs_estimate_f64.py shows that each lies further from the product than four tolerances on some plane of every size
that can show it.

Measured margins (test_acs_estimate_f64.py and test_gpu_acs_estimate.py print theirs with -s), over exactly the cases of
those files (KINDS x SIZES x DISTANCES, with candidates() of each size):
  DELTA_MEASURED  the largest |scaled - val| of the CPU double, in quantisation steps; DELTA is about four times that
                  (the convention of enc_fwd_f64.DELTA). The ambiguous band it leaves must hold less than MAX_BAND of the
                  values.
  RTOL_MEASURED   the largest relative deviation of an estimate from the reading under the product's roundings; RTOL is
                  four times that. On the flat plane only the lowest-frequency coefficient of each channel is not zero,
                  so the whole loss is |val - round(val)| of one value of some hundred steps, and its float32 error (1e-4
                  steps) against a remainder of a few hundredths is the estimate's: RTOL_FLAT_MEASURED, 24 times the
                  other kinds' figure, holds for FLAT_KINDS alone."""
import functools
import json
import os

import numpy as np

import adaptive_quant_f64 as A
import enc_fwd_f64 as F
import host_tables_np as T

_GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_constant_floats.json")))

# ac_strategy.h:130-167: blocks covered (x, y); quant_weights.h:352-382: the table kind
COVERED = {0: (1, 1), 4: (2, 2), 5: (4, 4), 6: (1, 2), 7: (2, 1), 8: (1, 4), 9: (4, 1), 10: (2, 4), 11: (4, 2),
           18: (8, 8), 19: (4, 8), 20: (8, 4)}
QUANT_KIND = {0: 0, 4: 4, 5: 5, 6: 6, 7: 6, 8: 7, 9: 7, 10: 8, 11: 8, 18: 11, 19: 12, 20: 12}
STRATEGIES = tuple(sorted(COVERED))

DELTA_MEASURED = 3.59e-4  # (the flat plane at 200x136, distance 0.5: a lowest-frequency value of 437 steps)
DELTA = 4 * DELTA_MEASURED
RTOL_MEASURED = 3.15e-6  # (the ramps at 200x136)
RTOL = 4 * RTOL_MEASURED
RTOL_FLAT_MEASURED = 7.61e-5  # (the flat plane at 200x136, distance 4)
RTOL_FLAT = 4 * RTOL_FLAT_MEASURED
FLAT_KINDS = ("flat",)
MAX_BAND = 1e-3
# The crafted planes are taken at a tenth of their level. The loop includes the lowest frequencies, whose values reach
# 8000 steps on the planes as crafted (distance 0.5, a 64x64 transform of Y around 0.45); a float32 chain is good to 6e-7
# of the value, 4.7e-3 steps there, and at four times that the ambiguous band of the noise plane held 2 % of its values. At a
# tenth the largest value is 780 steps and the band stays under MAX_BAND on every kind (the noise: 6.3e-4).
PLANE_SCALE = 0.1

SIZES = ((8, 8), (64, 64), (200, 136))  # (xsize, ysize): one block; one full tile; several tiles, partial on both axes
DISTANCES = (0.5, 1.0, 4.0)
KINDS = A.KINDS
MISREADINGS = ("x_weight_on_whole_sum", "quant_norm_plain_mean", "two_block_16_norm", "mask_offsets_exchanged",
               "channel_mul_without_power", "error_without_matrix", "error_with_inverse_matrix", "b_base_correlation_dropped",
               "entropy_mul_on_loss", "nbits_without_one", "tall_weights_not_transposed", "quant_norm_division_dropped")
# what a single 8x8 transform cannot show
NEEDS_SEVERAL_BLOCKS = ("x_weight_on_whole_sum", "quant_norm_plain_mean", "two_block_16_norm", "tall_weights_not_transposed")


def rtol(kind):
    return RTOL_FLAT if kind in FLAT_KINDS else RTOL


def planes(kind, size):
    """X, Y, B planes [3][ysize][xsize], float32, of one of KINDS at size = (xsize, ysize)."""
    return (A.crafted(kind, size[0], size[1]) * PLANE_SCALE).astype(np.float32)


def init_weights(distance):
    """:1111-1123 -> (info_loss_multiplier, zeros_mul, cost_delta)"""
    ratio = (distance + 0.13731742964354549) / (1.0 + 0.13731742964354549)
    return (1.2 * ratio ** 0.33677806662454718, 9.3089059022677905 * ratio ** 0.50990926717963703,
            10.833273317067883 * ratio ** 0.36702940662370243)


def ceil_log2_nonzero(v):
    v = np.asarray(v, np.int64)
    return np.ceil(np.log2(v)).astype(np.int64)  # (exact for the small integers met here: v <= 4097)


@functools.lru_cache(maxsize=None)
def matrix(strategy, tall_not_transposed=False):
    """config.dequant->Matrix of a strategy in the natural layout: [3][R][C], the weight of vertical frequency ky and
    horizontal frequency kx at [ky][kx]."""
    cx, cy = COVERED[strategy]
    R, C = 8 * cy, 8 * cx
    kind = QUANT_KIND[strategy]
    stored = 1.0 / T.compute_weights(kind, T.library_encoding(kind, _GOLDEN["quant_library"])).astype(np.float64)
    stored = stored.reshape(3, min(R, C), max(R, C))  # rows: the short side
    if R < C:
        return stored
    if R > C and tall_not_transposed:
        return stored.reshape(3, R, C)
    return stored.transpose(0, 2, 1)


def candidates(xs, ys, seed=11):
    """The candidates of one plane size, (strategy, bx, by, entropy_mul) each: every one of the twelve kinds at every
    position aligned to its own size that lies inside the planes (and so inside one 64x64 tile), then a few unaligned
    ones the walk's floating matches ask for: 16x16 at odd block offsets and 32x32 at offsets that are no multiple of 4,
    inside one tile. The multipliers are drawn from a few values around 1."""
    xb, yb = xs // 8, ys // 8
    rng = np.random.default_rng(seed + xs * 7 + ys)
    muls = (1.0, 0.85, 1.3, 0.5)
    out = []
    for s in STRATEGIES:
        cx, cy = COVERED[s]
        for by in range(0, yb - cy + 1, cy):
            for bx in range(0, xb - cx + 1, cx):
                out.append((s, bx, by))
    for s, offs in ((4, (1, 3, 5)), (5, (1, 2, 3))):
        cx, cy = COVERED[s]
        for ty in range(0, yb, 8):
            for tx in range(0, xb, 8):
                for oy in offs:
                    for ox in offs:
                        bx, by = tx + ox, ty + oy
                        if ox + cx <= 8 and oy + cy <= 8 and bx + cx <= xb and by + cy <= yb and (ox * 7 + oy + tx + ty) % 3 == 0:
                            out.append((s, bx, by))
    return [(s, bx, by, float(muls[rng.integers(len(muls))])) for s, bx, by in out]


def offsets(cands):
    """Where each candidate's 3 * R * C values start in the flat `scaled` array, and the total length."""
    area = np.array([192 * COVERED[c[0]][0] * COVERED[c[0]][1] for c in cands], np.int64)
    start = np.cumsum(area) - area
    return start, int(area.sum())


def estimate(xyb, quant_field, mask1x1, ytox, ytob, distance, cands, rounded=None, wrong=None):
    """-> (estimates [n], val flat as the product's `scaled`), float64. rounded: the roundings to evaluate the estimate
    under (flat, same layout), default np.rint(val). wrong: one of MISREADINGS, or None for the reading."""
    assert wrong is None or wrong in MISREADINGS
    xyb = np.asarray(xyb, np.float64)
    qf = np.asarray(quant_field, np.float64)
    mask = np.asarray(mask1x1, np.float64)
    ys, xs = xyb.shape[1:]
    tiles_x = (xs + 63) // 64
    info_mul, zeros_mul, cost_delta = init_weights(float(distance))
    start, total = offsets(cands)
    est, val_flat = np.zeros(len(cands)), np.zeros(total)
    strategy = np.array([c[0] for c in cands])
    mask_off = np.array([4.0, 0.0, 12.0] if wrong == "mask_offsets_exchanged" else [12.0, 0.0, 4.0])
    ch = np.array([8.2, 1.0, 1.03])
    channel_mul = ch if wrong == "channel_mul_without_power" else ch ** 8
    for s in np.unique(strategy):
        sel = np.flatnonzero(strategy == s)
        cx, cy = COVERED[int(s)]
        R, C, nb = 8 * cy, 8 * cx, cx * cy
        area = R * C
        bx = np.array([cands[i][1] for i in sel])
        by = np.array([cands[i][2] for i in sel])
        emul = np.array([cands[i][3] for i in sel], np.float64)
        n = len(sel)
        rows = by[:, None] * 8 + np.arange(R)[None]
        cols = bx[:, None] * 8 + np.arange(C)[None]
        px = xyb[:, rows[:, :, None], cols[:, None, :]]  # [3][n][R][C]
        coef = np.einsum("ur,cnrx,vx->cnuv", F.dct_matrix(R), px, F.dct_matrix(C), optimize=True)
        q = qf[(by[:, None, None] + np.arange(cy)[None, :, None]), (bx[:, None, None] + np.arange(cx)[None, None, :])].reshape(n, nb)
        norm16 = lambda v: np.mean(v ** 16, axis=1) ** (1.0 / 16.0)
        if nb == 1:
            qn = q[:, 0]
        elif nb == 2:
            qn = norm16(q) if wrong == "two_block_16_norm" else q.max(axis=1)
        else:
            qn = q.mean(axis=1) if wrong == "quant_norm_plain_mean" else norm16(q)
        tile = (by // 8) * tiles_x + bx // 8
        fx = np.asarray(ytox, np.float64).ravel()[tile] / 84.0
        fb = (0.0 if wrong == "b_base_correlation_dropped" else 1.0) + np.asarray(ytob, np.float64).ravel()[tile] / 84.0
        cmap = np.stack([fx, np.zeros(n), fb])  # [3][n]
        m = matrix(int(s), wrong == "tall_weights_not_transposed")[:, None]  # [3][1][R][C]
        val = (coef - coef[1][None] * cmap[:, :, None, None]) * ((1.0 / m) * qn[None, :, None, None])
        idx = start[sel][:, None] + np.arange(3 * area)[None]
        val_flat[idx] = val.transpose(1, 0, 2, 3).reshape(n, 3 * area)
        r = np.rint(val) if rounded is None else np.asarray(rounded, np.float64)[idx].reshape(n, 3, R, C).transpose(1, 0, 2, 3)
        diff = val - r
        e = diff if wrong == "error_without_matrix" else (diff / m if wrong == "error_with_inverse_matrix" else m * diff)
        pix = np.einsum("yu,cnuv,xv->cnyx", F.idct_matrix(R), e, F.idct_matrix(C), optimize=True)
        mk = mask[rows[:, :, None], cols[:, None, :]]  # [n][R][C]
        lossc = (((mk[None] + mask_off[:, None, None, None]) * pix) ** 8).sum(axis=(2, 3)) * channel_mul[:, None]  # [3][n]
        absr = np.abs(r)
        nz = (absr != 0).sum(axis=(2, 3))
        nbits = ceil_log2_nonzero(nz + 1) + (0 if wrong == "nbits_without_one" else 1)
        bits = cost_delta * np.sqrt(absr).sum(axis=(2, 3)) + zeros_mul * (ceil_log2_nonzero(nbits + 17) + nbits)  # [3][n]
        w = 1.0 + min(3.0, nb / 8.0) if nb >= 2 else 1.0
        if wrong == "x_weight_on_whole_sum":
            entropy, loss = w * bits.sum(axis=0), w * lossc.sum(axis=0)
        else:
            entropy, loss = w * bits[0] + bits[1] + bits[2], w * lossc[0] + lossc[1] + lossc[2]
        loss_scalar = (loss / area) ** 0.125 * area / (1.0 if wrong == "quant_norm_division_dropped" else qn)
        if wrong == "entropy_mul_on_loss":
            est[sel] = (entropy + info_mul * loss_scalar) * emul
        else:
            est[sel] = entropy * emul + info_mul * loss_scalar
    return est, val_flat
