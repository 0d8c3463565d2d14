"""A float64 NumPy reading of the reference's per-pixel masking (mask1x1), the image its AC-strategy search weighs the
reconstruction error with, written from the text of lib/jxl/enc_adaptive_quantization.cc (line numbers below are that
file's unless another is named) and sharing no code with csrc/enc/jxl_enc.cc, the HIP kernels or the oracle. It borrows
the crafted planes and ratio() of adaptive_quant_f64 (another reading).

  input      the Y plane padded to whole blocks, BEFORE the sharpening (AdaptiveQuantizationMap :664-705 runs on the same
             planes as the quant field).
  laplacian  ComputeTile :498-526. Per pixel base = 0.25 (down + up + left + right), a neighbour outside the plane being
             the pixel itself (x1 / x2 / y1 / y2 of :502-510); g = ratio<false>(Y + 0.019) (:127-145);
             v = 1 / (log1p(|g (Y - base)|) + 0.01).
  blur       Blur1x1Masking :634-662: Symmetric5 with the weights c = n, r = n k0, R = n k2, d = n k1, D = n k4, L = n k3,
             k = kFilterMask1x1 and n = 1 / (1 + 4 (k0 + k1 + k2 + k4 + 2 k3)). The initialiser lists them in the MEMBER
             order of WeightsSymmetric5 (convolve.h:30-40: c, r, R, d, D, L), which is not the reading order of the
             quadrant
                 c r R
                 r d L
                 R L D
             the struct's comment draws: the fifth value is D (the corner), the sixth L. The 25 weights sum to 1.
  border     convolve_symmetric5.cc:35-97, 128-176: rows and columns outside the plane are mirrored with the edge sample
             repeated (Mirror, image_ops.h:184-196: -1 -> 0, -2 -> 1).

MISREADINGS are deliberate wrong readings of the above; test_masking_1x1_f64.py shows that each lies further from the
product than the tolerance on the test planes, so the comparison could tell them from the right one.

Measured margins (test_masking_1x1_f64.py and test_gpu_masking_1x1.py print theirs with -s): the largest relative deviation
|product - reading| / |reading| of the CPU double and of the device over exactly the cases of those files (KINDS x SIZES);
a tolerance is four times its measurement. The float32 error sits in Y - base, half an ulp of Y (3e-8 at 0.5), times g,
against the 0.01 that v's denominator cannot fall below. g is of order 1 for a bright pixel and reaches its ceiling of 540
where Y + 0.019 is negative, so the planes fall into two classes and one tolerance for both would be a hundred times too wide
for the first:
  RTOL_MEASURED       the kinds whose Y + 0.019 stays positive
  RTOL_DARK_MEASURED  the kind that drives it below zero (DARK_KINDS: "negative")"""
import numpy as np

import adaptive_quant_f64 as A

K_FILTER = np.array([0.364911248, 0.05, 0.1688888021, 0.221069183, 0.306563504], np.float32).astype(np.float64)

RTOL_MEASURED = 6.51e-6  # (the steps at 200x136; the CPU double and the device alike)
RTOL = 4 * RTOL_MEASURED
RTOL_DARK_MEASURED = 5.85e-4  # (the negative plane at 200x136; the CPU double and the device alike)
RTOL_DARK = 4 * RTOL_DARK_MEASURED
DARK_KINDS = ("negative",)

SIZES = ((8, 8), (64, 64), (72, 40), (200, 136))  # (xsize, ysize): one block; one full tile of 64; partial tiles; several
KINDS = A.KINDS
MISREADINGS = ("quadrant_order", "blur_clamped", "blur_reflect_without_edge", "log_for_log1p", "gamma_offset_dropped",
               "ratio_inverted", "block_mask_offset", "centre_in_base")


def rtol(kind):
    return RTOL_DARK if kind in DARK_KINDS else RTOL


def laplacian(y, wrong=None):
    y = np.asarray(y, np.float64)
    p = np.pad(y, 1, mode="edge")
    base = 0.25 * (p[2:, 1:-1] + p[:-2, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:])
    if wrong == "centre_in_base":
        base = 0.2 * (4 * base + y)
    g = A.ratio(y + (0.0 if wrong == "gamma_offset_dropped" else 0.019), wrong == "ratio_inverted")
    d = np.abs(g * (y - base))
    d = np.log(np.maximum(d, 1e-300)) if wrong == "log_for_log1p" else np.log1p(d)
    return 1.0 / (d + (0.001 if wrong == "block_mask_offset" else 0.01))


def blur_kernel(wrong=None):
    k = K_FILTER
    n = 1.0 / (1.0 + 4 * (k[0] + k[1] + k[2] + k[4] + 2 * k[3]))
    c, r, R, d, D, L = n, n * k[0], n * k[2], n * k[1], n * k[4], n * k[3]
    if wrong == "quadrant_order":
        D, L = L, D
    q = np.array([[c, r, R], [r, d, L], [R, L, D]])
    i = np.abs(np.arange(-2, 3))
    return q[i[:, None], i[None, :]]


def masking_1x1(xyb, wrong=None):
    """X, Y, B planes [3][yp][xp] -> mask1x1 [yp][xp], float64. wrong: one of MISREADINGS, or None for the reading."""
    assert wrong is None or wrong in MISREADINGS
    v = laplacian(xyb[1], wrong)
    h, w = v.shape
    mode = {"blur_clamped": "edge", "blur_reflect_without_edge": "reflect"}.get(wrong, "symmetric")
    p = np.pad(v, 2, mode=mode)
    kern = blur_kernel(wrong)
    out = np.zeros_like(v)
    for dy in range(5):
        for dx in range(5):
            out += kern[dy, dx] * p[dy:dy + h, dx:dx + w]
    return out
