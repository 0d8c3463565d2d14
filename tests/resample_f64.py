"""A float64 reading of the resized binding (jxlhip_set_output_resized), written from the statement of its semantics and
sharing nothing with libjxl_amd/csrc/host/jxh_resample_plan.h: the separable antialiased triangle filter of a box of an
image, what torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) computes on the cropped
image. tests/test_resample_host.py holds it to torch itself and the host tables to it; tests/test_gpu_resample.py holds the
kernels to it.

Per axis, n_in the box extent and n_out the output extent:
    scale = n_in / n_out, support = max(scale, 1), center = scale * (i + 0.5)
    lo = max(0, trunc(center - support + 0.5)), hi = min(n_in, trunc(center + support + 0.5))
    w_j = max(0, 1 - |(j - center + 0.5) / support|) for j in [lo, hi), divided by their sum

`wrong` names one deliberate misreading (MISREADINGS); the tests show that each of them is far outside the error bar."""
import math

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32

MISREADINGS = ("align_corners", "no_antialias", "no_renormalise", "crop_after", "origin_off_by_one", "scales_exchanged",
               "floor_windows", "normalise_after_f32")


def axis_taps(n_in, n_out, wrong=None, scale=None, lo_limit=0, hi_limit=None, origin=0.0):
    """[(first, weights float64)] per output index. scale / lo_limit / hi_limit / origin serve the misreadings only: the scale
    if it is not n_in / n_out, the range of source indices that exist, and where the box starts inside that range."""
    if scale is None:
        scale = n_in / n_out
    if hi_limit is None:
        hi_limit = n_in
    rows = []
    if wrong == "align_corners":
        step = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        for i in range(n_out):
            x = i * step
            j = min(int(math.floor(x)), n_in - 1)
            f = x - j
            rows.append((j, np.array([1.0 - f, f] if j + 1 < n_in else [1.0])))
        return rows
    if wrong == "normalise_after_f32":
        # the weights live in float32 before they are normalised: scale, center and every w_j in float32 arithmetic, divided
        # by their float32 sum (torch's own float32 path). The float32 scale moves the centers.
        f = np.float32
        s32 = f(n_in) / f(n_out) if scale == n_in / n_out else f(scale)
        sup32 = max(s32, f(1))
        inv32 = f(1) / sup32
        for i in range(n_out):
            c32 = s32 * f(i + 0.5)
            lo = max(lo_limit, int(c32 - sup32 + f(0.5)))
            hi = min(hi_limit, int(c32 + sup32 + f(0.5)))
            w32 = np.array([max(f(0), f(1) - abs((f(j) - c32 + f(0.5)) * inv32)) for j in range(lo, hi)], f)
            rows.append((lo, (w32 / w32.sum(dtype=f)).astype(np.float64)))
        return rows
    support = 1.0 if wrong == "no_antialias" else max(scale, 1.0)
    inv = 1.0 / support
    for i in range(n_out):
        center = origin + scale * (i + 0.5)
        if wrong == "floor_windows":
            lo = max(lo_limit, int(math.floor(center - support)))  # (the window around floor(center): no half-sample shift)
            hi = max(lo + 1, min(hi_limit, int(math.floor(center + support))))
        else:
            lo = max(lo_limit, int(center - support + 0.5))  # (int() truncates)
            hi = min(hi_limit, int(center + support + 0.5))
        w = np.array([max(0.0, 1.0 - abs((j - center + 0.5) * inv)) for j in range(lo, hi)], np.float64)
        if wrong == "no_renormalise":
            w = w * inv  # (the weights of an inner row sum to `support`: edge rows are left short)
        else:
            w = w / w.sum()
        rows.append((lo, w))
    return rows


def axis_matrix(rows, n_in):
    m = np.zeros((len(rows), n_in), np.float64)
    for i, (lo, w) in enumerate(rows):
        m[i, lo:lo + len(w)] = w
    return m


def max_taps(n_in, n_out):
    return max(len(w) for _, w in axis_taps(n_in, n_out))


def resize(img, out_h, out_w, box=None, wrong=None):
    """img [H, W, C] (any float type; taken to float64), box = (x0, y0, xsize, ysize) or None -> [out_h, out_w, C] float64."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    x0, y0, bw, bh = box if box is not None else (0, 0, w, h)
    if wrong == "origin_off_by_one":
        x0, y0 = min(x0 + 1, w - bw), min(y0 + 1, h - bh)
    if wrong == "crop_after":  # the whole image resized at the box's scale, the taps reaching past the box's edge
        my = axis_matrix(axis_taps(h, out_h, scale=bh / out_h, lo_limit=0, hi_limit=h, origin=float(y0)), h)
        mx = axis_matrix(axis_taps(w, out_w, scale=bw / out_w, lo_limit=0, hi_limit=w, origin=float(x0)), w)
        src = img
    else:
        src = img[y0:y0 + bh, x0:x0 + bw]
        sy, sx = bh / out_h, bw / out_w
        if wrong == "scales_exchanged":
            sy, sx = sx, sy
        my = axis_matrix(axis_taps(bh, out_h, wrong, scale=sy), bh)
        mx = axis_matrix(axis_taps(bw, out_w, wrong, scale=sx), bw)
    return np.einsum("ij,jkc,lk->ilc", my, src, mx, optimize=True)


def bar(img, out_h, out_w, box=None):
    """The a-priori error bar of a float32 two-pass evaluation with weights rounded to float32:
    (tx + ty + 8) * 2^-24 * max(1, max |v| over the box). n-term float32 sums of convex weights contribute n * u each pass,
    the weights u / 2 each, the value between the passes one rounding."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    x0, y0, bw, bh = box if box is not None else (0, 0, w, h)
    v = np.abs(img[y0:y0 + bh, x0:x0 + bw])
    vmax = float(np.nanmax(v)) if v.size else 0.0
    return (max_taps(bw, out_w) + max_taps(bh, out_h) + 8) * U * max(1.0, vmax)


def emulate_f32(img, out_h, out_w, box=None):
    """A float32 two-pass evaluation with the reading's weights rounded to float32 (vertical pass first, sequential sums):
    shows on the CPU how far below the bar an honest float32 kernel stays."""
    img = np.asarray(img, np.float32)
    h, w = img.shape[:2]
    x0, y0, bw, bh = box if box is not None else (0, 0, w, h)
    src = img[y0:y0 + bh, x0:x0 + bw]
    tmp = np.zeros((out_h, bw, src.shape[2]), np.float32)
    for i, (lo, wt) in enumerate(axis_taps(bh, out_h)):
        acc = np.zeros(tmp.shape[1:], np.float32)
        for k, wk in enumerate(wt.astype(np.float32)):
            acc = (acc + wk * src[lo + k]).astype(np.float32)
        tmp[i] = acc
    out = np.zeros((out_h, out_w, src.shape[2]), np.float32)
    for i, (lo, wt) in enumerate(axis_taps(bw, out_w)):
        acc = np.zeros((out_h, src.shape[2]), np.float32)
        for k, wk in enumerate(wt.astype(np.float32)):
            acc = (acc + wk * tmp[:, lo + k]).astype(np.float32)
        out[:, i] = acc
    return out
