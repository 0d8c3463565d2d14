"""A reading of the spline feature: a quantised dictionary -> draw cache -> samples. Written from the reference's text and
from nothing under libjxl_amd/csrc or oracle/ (whose jxlo_splines.h is the host's jxh_splines.h under another name, so that
holding one to the other shows nothing):
  * lib/jxl/splines.cc:237-248 (the quantisation adjustment's two branches, the channel weights), :439-489
    (QuantizedSpline::Dequantize, the arithmetic: double deltas to control points, integer * (sqrt(1/2) for coefficient 0)
    * weight * inverse quant, then X += y_to_x Y and B += y_to_b Y; the area limits of :490-529 are decode-time refusals,
    not rendering, and stay out);
  * :300-342 (the centripetal Catmull-Rom: the end points extrapolated, knots sqrt(chord) apart, 16 samples per span, the
    last control point appended), :351-381 (ForEachEquallySpacedPoint: the first point, then one point per unit of arc
    length along the polyline, then the last polyline point with the length of the partial step as its intensity);
  * :707-713 (arc length = (n - 2) + the partial step; none: no segments: a single control point draws nothing);
  * :184-207 (SegmentsFromPoints: progress = min(1, k / arc length), colour and sigma = ContinuousIDCT at 31 * progress),
    :55-79 (ContinuousIDCT: sum of sqrt(2) * dct[i] * FastCosf(pi / 32 * i * (t + 1/2)); the multipliers are double
    products rounded to float), :129-171 (ComputeSegments: the checks on sigma, max_color with its floor of 0.01,
    kDistanceExp = 5, the llround row span, the segment's five numbers);
  * :719-755 (the per-row lists, in segment order); :82-127 (DrawSegment: the llround column span, clipped; the splat);
  * lib/jxl/base/fast_math-inl.h:95-124 (FastCosf), :126-148 (FastErff), restated as their formulas.
Both the host (jxh_splines.h InitSplineDrawCache), the oracle's copy of it and the HIP kernel (k_splines_add) are held to
it: tests/test_splines_f64.py, tests/test_gpu_splines_f64.py.

Everything takes `dtype`: float64 is the reading, float32 the same text rounded like the reference's floats (its constants
are the reference's float constants in both). The distance between the two is what the draw-cache bars are made of.

Formulation, on purpose unlike the host's loops: control points are two cumulative sums; the 15 inner samples of a span are
one array expression; ContinuousIDCT is a (points x 32) matrix of cosines summed along rows; the row lists come from a
stable sort of (row, segment) pairs; a row's splat is an array over its columns.

Bars (u = 2^-24).
Rendering (kernel or oracle against render() on the SAME float32 segment list): a-priori. Per segment and sample, with
d the distance, s = |inv_sigma|, c = 0.353553391, a+- = (d / 2 +- c) inv_sigma, E+- = erf~(a+-), f = E+ - E-:
  dx, dy: one rounding each; dx dx + dy dy fused or not: two more; sqrt: one      -> |delta d| <= 3 u d
  a+-: d / 2 is exact, the sum rounds once, the product once                     -> A+- = s (1.5 u d + u |d / 2 +- c|) + u |a+-|
  erf~(a) = 1 - 1 / q(|a|)^8, q a Horner form with positive terms: 4 roundings on q, then square, reciprocal, square,
  subtraction: 21 u on 1 / q^8 = 1 - |E|, one more on the result; its slope is at most 1.2
                                                                                 -> e+- = 21 u (1 - |E+-|) + u |E+-| + 1.2 A+-
  f: a difference that cancels, so the bound carries both terms, not |f|          -> F = e+ + e- + u |f|
  local = s4i (f f)                                                              -> L = |s4i| (2 |f| F + F^2) + 2 u |local|
  sample += colour * local, in list order, each sum rounded once                  -> sum_k |colour_k| L_k + u sum_k |partial sum_k|
render() returns that bound next to the samples. Span ends are exact: llround of one float32 difference of two given
floats, which the reading forms in float32 whatever `dtype` is.
Draw cache (host or oracle against draw_cache()): the walk is a long float32 recurrence; its bar is measured on the reading
itself: per case and field 4 x the largest |float32 reading - float64 reading| (DRAW_CACHE_DISTANCE below, recomputed and
printed by tests/test_splines_f64.py; the margin 4 is for the host's different, equally valid operation order). The
discrete results (point count, row spans) must agree except where the reading's llround argument is within the bar of a
half-integer; at most 1 % of a case's span ends may be that close.

Misreadings (MISREADINGS): named switches; tests/test_splines_f64.py shows each moves some case by more than ten bars.
Two notes. "tie_floor_plus_half" cannot show at a span end of 8.5 (floor(8.5 + 0.5) = 9 = llround); it shows where the
float sum v + 0.5 itself rounds up: v = 0.5 - 2^-25. "catmull_rom_no_sqrt" is the chordal spacing (for equal chords also the
uniform one)."""
import math

import numpy as np

U = 2.0 ** -24
F32 = np.float32
K_SQRT2, K_SQRT0_5 = F32(1.41421356237), F32(0.70710678118)      # dct_scales.h:15-16
CHANNEL_WEIGHT = [F32(0.0042), F32(0.075), F32(0.07), F32(0.3333)]  # splines.cc:248
IDCT_MULTIPLIERS = np.array([math.pi / 32 * i for i in range(32)]).astype(F32)  # splines.cc:60-68: double, then float
ERF_C = F32(0.353553391)

GEOMETRY_MISREADINGS = ("catmull_rom_no_sqrt", "samples_15", "samples_17", "no_extrapolated_ends", "dc_not_scaled", "idct_no_half",
                        "progress_by_count", "last_point_full", "last_point_dropped", "adjustment_swapped", "y_to_b_on_integers",
                        "distance_exp_3", "no_color_floor", "single_deltas")
RENDER_MISREADINGS = ("factor_not_squared", "inv_sigma_before_add", "tie_half_even", "tie_floor_plus_half")
MISREADINGS = GEOMETRY_MISREADINGS + RENDER_MISREADINGS


# ---- FastCosf, FastErff as formulas
def fast_cos(x, dtype=np.float64):
    """fast_math-inl.h:95-124: fold to [0, pi / 2], 2^(3/4) cos(x / 4) as a quartic, two angle doublings."""
    T = dtype
    x = np.asarray(x, T)
    two_pi, half_pi = T(F32(2 * math.pi)), T(F32(math.pi / 2))
    r = x - np.floor(x * T(F32(0.5 / math.pi))) * two_pi
    r = np.minimum(r, two_pi - r)
    above = r >= half_pi
    r = np.where(above, T(F32(math.pi)) - r, r) * T(0.25)
    x2 = r * r
    p = (x2 * x2) * T(F32(0.06960438)) + (x2 * T(F32(-0.84087373)) + T(F32(1.68179268)))
    p = p * p + T(F32(-1.414213562))
    p = p * p + T(-1)
    return np.where(above, -p, p).astype(T)


def fast_erf(x, dtype=np.float64):
    """fast_math-inl.h:126-148: 1 - 1 / ((((a x + b) x + c) x + d) x + 1)^4 squared once more, odd."""
    T = dtype
    x = np.asarray(x, T)
    a = np.abs(x)
    q = a * T(F32(7.77394369e-02)) + T(F32(2.05260015e-04))
    q = q * a + T(F32(2.32120216e-01))
    q = q * a + T(F32(2.77820801e-01))
    q = q * a + T(1)
    with np.errstate(over="ignore"):
        q = q * q  # (float32 overflows for |x| above about 1e5: 1 / inf = 0, the result +-1)
    inv = T(1) / q
    r = T(1) - inv * inv
    return np.where(x <= 0, -r, r).astype(T)


def llround(v, misread=None):
    """std::llround of one value: half away from zero, exactly (the fraction of a binary float is exact)."""
    if misread == "tie_half_even":
        return int(round(float(v)))
    if misread == "tie_floor_plus_half":
        return int(math.floor(type(v)(v + type(v)(0.5))))  # (the sum in the value's own precision)
    a = abs(float(v))
    whole = math.floor(a)
    n = int(whole) + (1 if a - whole >= 0.5 else 0)
    return -n if v < 0 else n


# ---- dictionary -> draw cache
def control_points(spline, misread=None):
    """splines.cc:451-476: integer control points from the start and the double deltas."""
    d = np.asarray(spline["deltas"], np.int64).reshape(-1, 2)
    steps = d if misread == "single_deltas" else np.cumsum(d, axis=0)
    return np.concatenate([np.asarray(spline["start"], np.int64).reshape(1, 2), np.asarray(spline["start"], np.int64) + np.cumsum(steps, axis=0)])


def dequantize(spline, adjustment, y_to_x, y_to_b, dtype=np.float64, misread=None):
    """splines.cc:478-489, 514-515. Returns (colour [3][32], sigma [32])."""
    T = dtype
    ge0 = adjustment >= 0
    if misread == "adjustment_swapped":
        ge0 = not ge0
        adjustment = -adjustment  # (each branch with the magnitude it was written for)
    inv_quant = T(1) / (T(1) + T(0.125) * T(adjustment)) if ge0 else T(1) - T(0.125) * T(adjustment)
    factor = np.ones(32, T)
    if misread != "dc_not_scaled":
        factor[0] = T(K_SQRT0_5)
    ints = np.asarray(spline["color"], np.int64).reshape(3, 32).astype(T)
    if misread == "y_to_b_on_integers":
        ints[2] = ints[2] + T(F32(y_to_b)) * ints[1]
    color = np.stack([ints[c] * factor * T(CHANNEL_WEIGHT[c]) * inv_quant for c in range(3)])
    color[0] = color[0] + T(F32(y_to_x)) * color[1]
    if misread != "y_to_b_on_integers":
        color[2] = color[2] + T(F32(y_to_b)) * color[1]
    sigma = np.asarray(spline["sigma"], np.int64).astype(T) * factor * T(CHANNEL_WEIGHT[3]) * inv_quant
    return color.astype(T), sigma.astype(T)


def catmull_rom(points, dtype=np.float64, misread=None):
    """splines.cc:300-342. points: [n][2]; returns the polyline [m][2]."""
    T = dtype
    p = np.asarray(points, T)
    if len(p) == 1:
        return p.copy()
    n = {"samples_15": 15, "samples_17": 17}.get(misread, 16)
    if misread != "no_extrapolated_ends":
        p = np.concatenate([(p[0] + (p[0] - p[1]))[None], p, (p[-1] + (p[-1] - p[-2]))[None]])
    out = []
    frac = (np.arange(1, n).astype(T) / T(n))[:, None]
    for s in range(len(p) - 3):
        q = p[s:s + 4]
        chord = np.hypot(q[1:, 0] - q[:-1, 0], q[1:, 1] - q[:-1, 1]).astype(T)
        d = chord if misread == "catmull_rom_no_sqrt" else np.sqrt(chord)
        t = [T(0), d[0], d[0] + d[1], (d[0] + d[1]) + d[2]]
        tt = d[0] + frac * d[1]
        a = [q[k] + ((tt - t[k]) / d[k]) * (q[k + 1] - q[k]) for k in range(3)]
        b = [a[k] + ((tt - t[k]) / (d[k] + d[k + 1])) * (a[k + 1] - a[k]) for k in range(2)]
        out.append(q[1][None])
        out.append(b[0] + ((tt - t[1]) / d[1]) * (b[1] - b[0]))
    out.append(p[-2][None])
    return np.concatenate(out).astype(T)


def equally_spaced(poly, dtype=np.float64, misread=None):
    """splines.cc:351-381. Returns (points [m][2], intensity [m])."""
    T = dtype
    poly = np.asarray(poly, T)
    pts, mult = [poly[0]], [T(1)]
    cur, nxt = poly[0], 0
    while nxt < len(poly):
        prev, walked = cur, T(0)
        while True:
            if nxt == len(poly):
                if misread != "last_point_dropped":
                    pts.append(prev)
                    mult.append(T(1) if misread == "last_point_full" else walked)
                return np.array(pts, T), np.array(mult, T), walked
            v = poly[nxt] - prev
            step = np.sqrt(v[0] * v[0] + v[1] * v[1])
            if walked + step >= T(1):
                cur = prev + ((T(1) - walked) / step) * v
                pts.append(cur)
                mult.append(T(1))
                break
            walked = walked + step
            prev = poly[nxt]
            nxt += 1
    raise AssertionError("unreachable: the walk ends at the polyline's end")


def continuous_idct(dct, t, dtype=np.float64, misread=None):
    """splines.cc:55-79 at every position of t."""
    T = dtype
    shifted = np.asarray(t, T) if misread == "idct_no_half" else np.asarray(t, T) + T(0.5)
    cos = fast_cos(IDCT_MULTIPLIERS.astype(T)[None, :] * shifted[:, None], T)
    return (T(K_SQRT2) * (np.asarray(dct, T)[None, :] * cos)).sum(axis=1, dtype=T)


def draw_cache(dictionary, xsize, ysize, y_to_x, y_to_b, dtype=np.float64, misread=None):
    """Splines::InitializeDrawCache (splines.cc:657-758). dictionary: {"adjustment": int, "splines": [{"start": (x, y),
    "deltas": [(ddx, ddy), ...], "color": [3][32] ints, "sigma": [32] ints}, ...]}. Returns a dict: segments [n][8] (centre x,
    y, maximum distance, 1 / sigma, sigma / 4 * intensity, colour X, Y, B), spans [n][2] (first row, one past the last),
    span_args [n][2] (what was rounded for the two: centre y -+ maximum distance, before the + 1 and the clip), points (number
    of points per spline), row_start [ysize + 1], row_segments."""
    T = dtype
    assert misread is None or misread in MISREADINGS
    segs, spans, args, counts = [], [], [], []
    for sp in dictionary["splines"]:
        color_dct, sigma_dct = dequantize(sp, dictionary["adjustment"], y_to_x, y_to_b, T, misread)
        pts, mult, partial = equally_spaced(catmull_rom(control_points(sp, misread), T, misread), T, misread)
        counts.append(len(pts))
        arc = T(len(pts) - 2) + (mult[-1] if misread != "last_point_dropped" else partial)
        if not arc > 0:
            continue
        k = np.arange(len(pts)).astype(T)
        progress = np.minimum(T(1), k / T(max(1, len(pts) - 1)) if misread == "progress_by_count" else k * (T(1) / arc))
        t = T(31) * progress
        color = np.stack([continuous_idct(color_dct[c], t, T, misread) for c in range(3)], axis=1)
        sigma = continuous_idct(sigma_dct, t, T, misread)
        exp = T(3) if misread == "distance_exp_3" else T(5)
        for i in range(len(pts)):
            s, m = sigma[i], mult[i]
            with np.errstate(divide="ignore"):
                if not (np.isfinite(s) and s != 0 and np.isfinite(T(1) / s) and np.isfinite(m)):
                    continue
            mc = np.abs(color[i] * m).max()
            if misread != "no_color_floor":
                mc = max(T(0.01) if T is np.float64 else T(F32(0.01)), mc)
            mc = T(mc)
            with np.errstate(divide="ignore", invalid="ignore"):
                maxd = np.sqrt(T(-2) * s * s * (np.log(T(F32(0.1))) * exp - np.log(mc)))
            if not np.isfinite(maxd):
                continue
            lo, hi = pts[i][1] - maxd, pts[i][1] + maxd
            y0, y1 = max(llround(lo), 0), min(llround(hi) + 1, ysize)
            if y1 <= y0:
                continue
            segs.append([pts[i][0], pts[i][1], maxd, T(1) / s, T(0.25) * s * m, color[i][0], color[i][1], color[i][2]])
            spans.append((y0, y1))
            args.append((lo, hi))
    segments = np.array(segs, T).reshape(-1, 8)
    spans = np.array(spans, np.int64).reshape(-1, 2)
    row_start, row_segments = row_lists(spans, ysize)
    return dict(segments=segments, spans=spans, span_args=np.array(args, T).reshape(-1, 2), points=counts, row_start=row_start,
                row_segments=row_segments)


def row_lists(spans, ysize):
    """splines.cc:719-755: row y lists the segments whose span holds y, in segment order."""
    pairs = [(y, i) for i, (y0, y1) in enumerate(spans) for y in range(y0, y1)]
    pairs.sort(key=lambda p: p[0])  # (stable: segment order within a row)
    rows = np.array([p[0] for p in pairs], np.int64)
    row_start = np.searchsorted(rows, np.arange(ysize + 1)).astype(np.uint32)
    return row_start, np.array([p[1] for p in pairs], np.uint32)


# ---- draw cache -> samples
def render(planes, segments, row_start, row_segments, y_begin=0, y_end=None, dtype=np.float64, misread=None):
    """DrawSegments / DrawSegment (splines.cc:82-127, 173-182) on planes [3][ysize][xsize], rows y_begin .. y_end, from a
    float32 segment list (or the reading's float64 one, whose span ends are then rounded from float64 sums). Returns (planes after, the a-priori float32 bound on every sample: see the module docstring)."""
    T = dtype
    assert misread is None or misread in MISREADINGS
    out = np.array(planes, T)
    ysize, xsize = out.shape[1:]
    y_end = ysize if y_end is None else y_end
    bound = np.zeros(out.shape, np.float64)
    partial = np.abs(np.asarray(planes, np.float64))
    seg32 = np.asarray(segments).reshape(-1, 8)  # (a float32 list as given; the reading's own float64 cache unrounded)
    assert seg32.dtype in (F32, np.float64)
    lists = [np.asarray(row_segments[row_start[y]:row_start[y + 1]], np.int64) for y in range(y_begin, y_end)]
    if all((np.diff(l) > 0).all() for l in lists):
        # every row's list ascends: segment by segment over the rows that name it adds to each sample in the same order
        rows_of = {}
        for y, l in zip(range(y_begin, y_end), lists):
            for i in l:
                rows_of.setdefault(int(i), []).append(y)
        work = [(i, np.array(rows_of[i])) for i in sorted(rows_of)]
    else:
        work = [(int(i), np.array([y])) for y, l in zip(range(y_begin, y_end), lists) for i in l]
    for i, ys in work:
        g = seg32[i]
        start, end = llround(g[0] - g[2], misread), llround(g[0] + g[2], misread)  # (float32 differences, as given)
        if end < 0 or start >= xsize:
            continue
        x0, x1 = max(0, start), min(xsize, end + 1)
        if x0 >= x1:
            continue
        cx, cy, inv_sigma, s4i = T(g[0]), T(g[1]), T(g[3]), T(g[4])
        dx, dy = (np.arange(x0, x1).astype(T) - cx)[None, :], (ys.astype(T) - cy)[:, None]
        d = np.sqrt(dx * dx + dy * dy)
        if misread == "inv_sigma_before_add":
            ap, am = d * T(0.5) + T(ERF_C) * inv_sigma, d * T(0.5) - T(ERF_C) * inv_sigma
        else:
            ap, am = (d * T(0.5) + T(ERF_C)) * inv_sigma, (d * T(0.5) - T(ERF_C)) * inv_sigma
        ep, em = fast_erf(ap, T), fast_erf(am, T)
        f = ep - em
        local = s4i * f if misread == "factor_not_squared" else s4i * (f * f)
        # the bound, in float64 whatever T is
        d64, s = np.abs(np.asarray(d, np.float64)), abs(float(inv_sigma))
        e = 0.0
        for a_, e_, sign in ((ap, ep, 1.0), (am, em, -1.0)):
            arg = s * (1.5 * U * d64 + U * np.abs(d64 / 2 + sign * float(ERF_C))) + U * np.abs(np.asarray(a_, np.float64))
            e = e + 21 * U * (1 - np.abs(np.asarray(e_, np.float64))) + U * np.abs(np.asarray(e_, np.float64)) + 1.2 * arg
        F = e + U * np.abs(np.asarray(f, np.float64))
        L = abs(float(s4i)) * (2 * np.abs(np.asarray(f, np.float64)) * F + F * F) + 2 * U * np.abs(np.asarray(local, np.float64))
        at = (ys[:, None], np.arange(x0, x1)[None, :])
        for c in range(3):
            col = T(g[5 + c])
            out[c][at] = col * local + out[c][at]
            partial[c][at] += np.abs(float(col) * np.asarray(local, np.float64))
            bound[c][at] += abs(float(col)) * L + U * partial[c][at]
    return out, bound


# End to end (dictionary -> samples on planes of zeros): the largest |float32 reading - float64 reading| of any sample, per
# case, measured and printed by tests/test_splines_f64.py::test_reading_end_to_end_float32_against_float64; a decoder's planes
# are held to 4 times these.
END_TO_END_DISTANCE = {'four_point_curve': 6.44e-05, 'hairpin': 4.86e-05, 'closed_loop': 4.38e-05, 'sigma_changes_sign': 0.000167,
                       'two_strokes_cmap': 6.32e-05}

# The largest |float32 reading - float64 reading| per case of tests/test_splines_f64.py and field (centre, maximum
# distance, 1 / sigma relative, sigma / 4 * intensity, colour), measured by test_reading_float32_against_float64 there,
# which prints them; a draw cache is held to 4 times these.
DRAW_CACHE_MARGIN = 4.0
DRAW_CACHE_DISTANCE = {
    'line_220': {'centre': 0, 'maximum_distance': 1.43e-06, 'inv_sigma': 3.32e-08, 'sigma_over_4_times_intensity': 8.2e-08, 'colour': 3.3e-06},
    'line_60_down': {'centre': 0, 'maximum_distance': 5.62e-06, 'inv_sigma': 4.48e-07, 'sigma_over_4_times_intensity': 2.3e-07, 'colour': 7.78e-06},
    'one_pixel': {'centre': 0, 'maximum_distance': 1.43e-06, 'inv_sigma': 3.32e-08, 'sigma_over_4_times_intensity': 8.2e-08, 'colour': 3.3e-06},
    'single_point': {'centre': 0, 'maximum_distance': 0, 'inv_sigma': 0, 'sigma_over_4_times_intensity': 0, 'colour': 0},
    'diagonal': {'centre': 0.000129, 'maximum_distance': 0.000153, 'inv_sigma': 7.94e-07, 'sigma_over_4_times_intensity': 0.000146, 'colour': 8.51e-06},
    'four_point_curve': {'centre': 7.98e-05, 'maximum_distance': 6.03e-05, 'inv_sigma': 9.98e-09, 'sigma_over_4_times_intensity': 5.02e-05, 'colour': 8.86e-06},
    'two_point_stroke': {'centre': 6.37e-05, 'maximum_distance': 3e-05, 'inv_sigma': 6.45e-07, 'sigma_over_4_times_intensity': 2.33e-05, 'colour': 1.75e-06},
    'hairpin': {'centre': 0.000101, 'maximum_distance': 1.33e-05, 'inv_sigma': 1.19e-06, 'sigma_over_4_times_intensity': 1.46e-05, 'colour': 7.59e-06},
    'closed_loop': {'centre': 0.000139, 'maximum_distance': 6.88e-05, 'inv_sigma': 2.28e-07, 'sigma_over_4_times_intensity': 4.39e-05, 'colour': 1.09e-05},
    'across_the_frame': {'centre': 0, 'maximum_distance': 9.35e-06, 'inv_sigma': 3.09e-07, 'sigma_over_4_times_intensity': 3.84e-07, 'colour': 8.12e-06},
    'sigma_changes_sign': {'centre': 0.000169, 'maximum_distance': 0.000117, 'inv_sigma': 0.0244, 'sigma_over_4_times_intensity': 0.000137, 'colour': 1.77e-05},
    'two_strokes_vardct': {'centre': 7.98e-05, 'maximum_distance': 4.26e-05, 'inv_sigma': 6.45e-07, 'sigma_over_4_times_intensity': 3.26e-05, 'colour': 1.19e-05},
    'two_strokes_cmap': {'centre': 7.98e-05, 'maximum_distance': 1.89e-05, 'inv_sigma': 1.46e-06, 'sigma_over_4_times_intensity': 1.46e-05, 'colour': 5.57e-06},
    'upsampled_frame': {'centre': 3.59e-05, 'maximum_distance': 2.97e-05, 'inv_sigma': 3.3e-07, 'sigma_over_4_times_intensity': 2.67e-05, 'colour': 1.28e-05},
}
