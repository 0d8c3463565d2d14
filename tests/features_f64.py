"""A reading of the two image features behind the loop filters that had none: upsampling by 2 / 4 / 8 (float64) and
noise synthesis (the generator bit-exact in uint64, the rest float64). Written from the reference's text and from nothing
under libjxl_amd/csrc or oracle/:
  * lib/jxl/render_pipeline/stage_upsampling.cc:59-84 (the N x N kernels out of the symmetric weight matrix), :147-206 (the
    minimum / maximum of the 5 x 5 window), :243-261 (the 25-tap sum and the clamp); image_metadata.cc:87-214 (the weights
    are the upper triangle, row by row); low_memory_render_pipeline.cc / image_ops.h:184-196 (edges mirror, and a frame of
    one or two samples mirrors more than once);
  * lib/jxl/xorshift128plus-inl.h:46-95 (seeding, one step), dec_noise.cc:44-106 (bits to [1, 2), whole 16-float steps while
    x + 16 < w and then always one more, three planes from one generator) and :120-152 (one generator per 256 x 256 square of
    the IMAGE, seeded with the two frame indices and the square's origin);
  * lib/jxl/render_pipeline/stage_noise.cc:258-300 (the 5 x 5 high-pass), :62-129 (strength from the 8-point table),
    :141-169 and :186-230 (the 1/128 : 127/128 mix, the base correlation); dec_cache.cc:198-219 (patches, splines,
    upsampling, then noise).
What it shares with the rest of the suite: the default weights, as DATA (tests/golden/ref_constant_floats.json, which
test_kats.py holds both .inc copies to). Both the oracle (oracle/jxlo_render.h Upsample, AddNoise) and the HIP kernels
(k_upsample_color, k_upsample_plane, k_noise_random, k_noise_add) are held to it.

Formulation, on purpose unlike the kernels': the kernels are slices of the full symmetric matrix, the image is padded once
by np.pad and the 25 taps are one tensor contraction over sliding windows; the generator runs all its steps for a square
first and the planes are reshapes of that; the high-pass is a box sum of the padded plane; the strength is np.interp.

Bars (u = 2^-24, the unit roundoff of binary32).
Upsampling: |x - reading| <= 26 u mag + 2 u |reading|, mag = sum |w_i v_i|: the a-priori bound of a 25-term binary32 dot
product in any order, fused or not ((1 + u)^26 - 1 < 26 u (1 + 2e-6)); the clamp is 1-Lipschitz and its bounds are inputs;
the second term is the rounding of the result to binary32. Measured: the oracle's largest distance on the cases of
test_features_f64.py is 0.0822 of this bar, so 4 x 0.0822 = 0.329 of it is the bar in use (UPSAMPLE_BAR_SCALE).
Noise: the raw planes are exact. For the planes, with S the sum of the 24 neighbours, p the centre (all in [1, 2)):
  others: 23 rounded additions of partial sums <= S            -> 23 u S
  t = 0.16 others + (-3.84) p: two products, one sum           -> 0.16 * 23 u S + 2 u (0.16 S + 3.84 p) = u (4 S + 7.68 p)
  rnd = 0.22 t                                                 -> E = 0.22 u (4 S + 7.68 p) + u |rnd|
  m = rnd_c / 128 + 127/128 rnd_2 (the first product is exact) -> E_m = E_c / 128 + 127/128 E_2 + 2 u (|rnd_c| / 128 + |rnd_2|)
  x = (Y -+ X) / 2, scaled = 6 x                               -> 12 u |x| on `scaled`; the table is continuous and piecewise
  linear in `scaled` with slopes <= D = the largest table step (<= 6 D in x), its evaluation (hi - lo) * frac + lo rounds
  three times                                                  -> E_s = 12 u |x| D + 3 u (max |lut| + D)
  red = s m                                                    -> E_red = E_s |m| + s E_m + u |red|   (green alike)
  rg = red + green, d = red - green                            -> E_rg = E_red + E_green + u |rg|, E_d alike
  X' = (ytox rg + d) + X                                       -> |ytox| E_rg + E_d + 2 u (|ytox rg| + |d|) + 2 u |X'|
  Y' = Y + rg                                                  -> E_rg + 2 u |Y'|
  B' = ytob rg + B                                             -> |ytob| E_rg + u |ytob rg| + 2 u |B'|
An error e_X, e_Y, e_B on the input planes (the upsampling's bar, when the noise follows it) adds e_c + the strength's
slope times it: 3 D (e_X + e_Y) (|m_r| + |m_g|) times (1 + |ytox|), 1, |ytob| for X, Y, B.
Measured: the oracle's largest distance on the cases of test_features_f64.py is 0.206 of this bar, so the derived bar is the one in use (NOISE_BAR_SCALE = 1).
The bars the tests use are the derived ones times the *_BAR_SCALE below: where the derived bar is more than 8 times the
oracle's largest distance, 4 times that distance replaces it. No kernel's result went into them."""
import functools
import json
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24

# measured by tests/test_features_f64.py::test_oracle_sits_within_the_bars (it prints them): the oracle's largest
# |oracle - reading| / derived bar. Where that is below 1 / 8, the bar in use is 4 times the oracle's distance.
ORACLE_UPSAMPLE_DISTANCE = 0.0822
ORACLE_NOISE_DISTANCE = 0.206
UPSAMPLE_BAR_SCALE = 1.0 if ORACLE_UPSAMPLE_DISTANCE >= 1 / 8 else 4 * ORACLE_UPSAMPLE_DISTANCE
NOISE_BAR_SCALE = 1.0 if ORACLE_NOISE_DISTANCE >= 1 / 8 else 4 * ORACLE_NOISE_DISTANCE

UPSAMPLE_MISREADINGS = ("edge_replicate", "kernel_not_flipped", "triangle_row_major_full", "no_clamp", "clamp_3x3")
NOISE_MISREADINGS = ("noise_no_extra_step", "noise_origin_swapped", "noise_planes_interleaved", "noise_mirror_per_square",
                     "noise_strength_unclamped_end")
ORDER_MISREADINGS = ("noise_before_upsampling",)
MISREADINGS = UPSAMPLE_MISREADINGS + NOISE_MISREADINGS + ORDER_MISREADINGS


@functools.lru_cache(maxsize=None)
def default_weights(n):
    """The default upper triangle of factor n, as float32."""
    f = json.load(open(os.path.join(_GOLDEN, "ref_constant_floats.json")))
    return np.asarray(f["upsampling_weights%d" % n], np.float32)


def upsampling_kernels(n, weights=None, misread=None):
    """[n][n][5][5] float32: kernel [oy][ox] makes output sample (n y + oy, n x + ox) from the window around (y, x).
    The coded weights are the upper triangle, row by row, of a symmetric matrix of side 5 n / 2 whose entry
    [5 ky + py][5 kx + px] is tap (py, px) of kernel (ky, kx) for ky, kx < n / 2; the far half in x is the near half with
    kernels and taps mirrored in x, and the same in y."""
    w = default_weights(n) if weights is None else np.asarray(weights, np.float32)
    h = n // 2
    side = 5 * h
    assert w.shape == (side * (side + 1) // 2,)
    m = np.zeros((side, side), np.float32)
    iu = np.triu_indices(side)
    if misread == "triangle_row_major_full":  # (row r of the triangle taken to start at r * side; past the end wraps)
        m[iu] = w[(iu[0] * side + (iu[1] - iu[0])) % len(w)]
    else:
        m[iu] = w
    m = np.triu(m) + np.triu(m, 1).T
    q = m.reshape(h, 5, h, 5).transpose(0, 2, 1, 3)  # [ky][kx][py][px]
    k = np.empty((n, n, 5, 5), np.float32)
    k[:h, :h] = q
    if misread == "kernel_not_flipped":  # (the far kernels in mirrored order, their taps not mirrored)
        k[:h, h:] = q[:, ::-1]
        k[h:] = k[:h][::-1]
    else:
        k[:h, h:] = q[:, ::-1, :, ::-1]
        k[h:] = k[:h][::-1, :, ::-1, :]
    return k


def _pad_mirror(a, pad, mode="symmetric"):
    """`pad` samples on every side; mirrored edges repeat the edge sample, and a plane smaller than the pad is mirrored
    again (each round adds at most the size the plane has by then)."""
    a = np.asarray(a)
    left = [pad, pad]
    while any(left):
        step = [min(left[0], a.shape[0]), min(left[1], a.shape[1])]
        a = np.pad(a, ((step[0], step[0]), (step[1], step[1])), mode=mode)
        left = [left[0] - step[0], left[1] - step[1]]
    return a


def upsample(plane, n, kernels, out_xs, out_ys, misread=None):
    """plane [ys][xs] -> (out [out_ys][out_xs], mag [out_ys][out_xs]) in float64; mag = sum |w_i v_i| of the sample's 25
    taps. ceil(out / n) must be the plane's size."""
    p = np.asarray(plane, np.float64)
    ys, xs = p.shape
    assert -(-out_xs // n) == xs and -(-out_ys // n) == ys
    k = np.asarray(kernels, np.float64).reshape(n, n, 5, 5)
    win = sliding_window_view(_pad_mirror(p, 2, "edge" if misread == "edge_replicate" else "symmetric"), (5, 5))  # [y][x][py][px]
    out = np.einsum("yxpq,abpq->yaxb", win, k).reshape(ys * n, xs * n)
    mag = np.einsum("yxpq,abpq->yaxb", np.abs(win), np.abs(k)).reshape(ys * n, xs * n)
    if misread != "no_clamp":
        box = win[:, :, 1:4, 1:4] if misread == "clamp_3x3" else win
        lo = np.repeat(np.repeat(box.min(axis=(2, 3)), n, 0), n, 1)
        hi = np.repeat(np.repeat(box.max(axis=(2, 3)), n, 0), n, 1)
        out = np.clip(out, lo, hi)
    return out[:out_ys, :out_xs], mag[:out_ys, :out_xs]


def upsample_bar(out, mag):
    return UPSAMPLE_BAR_SCALE * (26 * U * mag + 2 * U * np.abs(out))


# ---- noise
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _seed_lanes(hi, lo):
    """Eight lanes: lane 0 from (hi << 32) + lo + the golden ratio, lane i from lane i - 1."""
    out = np.empty(8, np.uint64)
    with np.errstate(over="ignore"):
        z = np.array([(int(hi) << 32) + int(lo)], np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    for i in range(8):
        z = _splitmix(z)
        out[i] = z[0]
    return out


def xorshift_single_seed(seed, steps):
    """The one-seed constructor (xorshift128plus-inl.h:36-44, what xorshift128plus_test.cc seeds): [steps][8] uint64."""
    s0, s1 = np.empty(8, np.uint64), np.empty(8, np.uint64)
    with np.errstate(over="ignore"):
        z = np.array([seed], np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    for i in range(8):
        z = _splitmix(z)
        s0[i] = z[0]
        z = _splitmix(z)
        s1[i] = z[0]
    return _run(s0, s1, steps)


def _run(s0, s1, steps):
    """`steps` steps of the eight xorshift128+ lanes: [steps][8] uint64."""
    out = np.empty((steps, 8), np.uint64)
    a, b = s0.copy(), s1.copy()
    with np.errstate(over="ignore"):
        for t in range(steps):
            out[t] = a + b
            x = a ^ (a << np.uint64(23))
            a = b
            b = x ^ b ^ (x >> np.uint64(18)) ^ (b >> np.uint64(5))
    return out


def noise_random(xs, ys, seed0, seed1, misread=None):
    """[3][ys][xs] uint32: the bit patterns of the raw random planes (binary32 values in [1, 2))."""
    out = np.zeros((3, ys, xs), np.uint32)
    for y0 in range(0, ys, 256):
        for x0 in range(0, xs, 256):
            w, h = min(256, xs - x0), min(256, ys - y0)
            origin = (y0, x0) if misread == "noise_origin_swapped" else (x0, y0)
            # whole steps while x + 16 < w, then always one more: (w - 1) // 16 + 1 steps of 16 floats for a row of w >= 1
            per_row = (w - 1) // 16 if misread == "noise_no_extra_step" else (w - 1) // 16 + 1
            per_row = max(per_row, 1)
            bits = _run(_seed_lanes(seed0, seed1), _seed_lanes(*origin), 3 * h * per_row)
            halves = np.ascontiguousarray(bits.astype("<u8")).view("<u4")  # the low half of a lane comes first
            f = (halves >> np.uint32(9)) | np.uint32(0x3F800000)
            if misread == "noise_planes_interleaved":
                sq = f.reshape(h, 3, per_row * 16).transpose(1, 0, 2)
            else:
                sq = f.reshape(3, h, per_row * 16)
            col = np.arange(w)
            if misread == "noise_no_extra_step":  # (the rest of the row repeats the last step instead of taking a new one)
                col = np.where(col < per_row * 16, col, (per_row - 1) * 16 + col % 16)
            out[:, y0:y0 + h, x0:x0 + w] = sq[:, :, col]
    return out


def _f32(v):
    return np.float64(np.float32(v))


def _box25(raw, misread):
    """Sum of the 5 x 5 window around every sample of raw [ys][xs], the plane mirrored at the image's edges."""
    if misread == "noise_mirror_per_square":
        out = np.empty_like(raw)
        for y0 in range(0, raw.shape[0], 256):
            for x0 in range(0, raw.shape[1], 256):
                out[y0:y0 + 256, x0:x0 + 256] = _box25(raw[y0:y0 + 256, x0:x0 + 256], None)
        return out
    p = _pad_mirror(raw, 2)
    rows = sliding_window_view(p, 5, axis=0).sum(axis=-1)
    return sliding_window_view(rows, 5, axis=1).sum(axis=-1)


def noise_strength(lut, x, misread=None):
    """The 8-point table at 6 x: clipped to the table's ends (below 0 the first point, from 7 on the last), linear between
    the points, and the result clipped to [0, 1]."""
    lut = np.asarray(lut, np.float64)
    scaled = 6.0 * np.asarray(x, np.float64)
    v = np.interp(scaled, np.arange(8.0), lut)
    if misread == "noise_strength_unclamped_end":  # (the last segment runs on)
        v = np.where(scaled >= 7.0, lut[6] + (lut[7] - lut[6]) * (scaled - 6.0), v)
    return np.clip(v, 0.0, 1.0)


def noise_add(xyb, raw, lut, ytox, ytob, misread=None, in_err=None):
    """xyb [3][ys][xs] (X, Y, B), raw [3][ys][xs] float32 random planes -> (planes with the noise, their bar), float64.
    in_err: a bound on the error xyb already carries (added to the bar with the strength's slope)."""
    v = np.asarray(xyb, np.float64)
    r = np.asarray(raw, np.float32).astype(np.float64)
    lut = np.asarray(lut, np.float32).astype(np.float64)
    ytox, ytob = _f32(ytox), _f32(ytob)
    k_others, k_centre, k_norm = _f32(0.16), _f32(-3.84), _f32(0.22)
    box = np.stack([_box25(r[c], misread) for c in range(3)])
    others = box - r
    rnd = k_norm * (k_others * others + k_centre * r)
    e_rnd = 0.22 * U * (4 * others + 7.68 * r) + U * np.abs(rnd)
    a, b = 1.0 / 128, 127.0 / 128
    step = np.abs(np.diff(lut)).max()
    top = np.abs(lut).max() + step
    vx, vy, vb = v
    m, e_m, s, e_s = {}, {}, {}, {}
    for name, c, x in (("r", 0, (vy + vx) * 0.5), ("g", 1, (vy - vx) * 0.5)):
        m[name] = a * rnd[c] + b * rnd[2]
        e_m[name] = a * e_rnd[c] + b * e_rnd[2] + 2 * U * (a * np.abs(rnd[c]) + np.abs(rnd[2]))
        s[name] = noise_strength(lut, x, misread)
        e_s[name] = 12 * U * np.abs(x) * step + 3 * U * top
    red, green = s["r"] * m["r"], s["g"] * m["g"]
    e_red = e_s["r"] * np.abs(m["r"]) + s["r"] * e_m["r"] + U * np.abs(red)
    e_green = e_s["g"] * np.abs(m["g"]) + s["g"] * e_m["g"] + U * np.abs(green)
    rg, d = red + green, red - green
    e_rg = e_red + e_green + U * np.abs(rg)
    e_d = e_red + e_green + U * np.abs(d)
    out = np.stack([(ytox * rg + d) + vx, vy + rg, ytob * rg + vb])
    bar = np.stack([abs(ytox) * e_rg + e_d + 2 * U * (np.abs(ytox * rg) + np.abs(d)) + 2 * U * np.abs(out[0]),
                    e_rg + 2 * U * np.abs(out[1]),
                    abs(ytob) * e_rg + U * np.abs(ytob * rg) + 2 * U * np.abs(out[2])])
    bar = NOISE_BAR_SCALE * bar
    if in_err is not None:
        e = np.asarray(in_err, np.float64)
        slope = 3 * step * (e[0] + e[1]) * (np.abs(m["r"]) + np.abs(m["g"]))
        bar = bar + e + np.stack([(1 + abs(ytox)) * slope, slope, abs(ytob) * slope])
    return out, bar


def noise(xyb, seed0, seed1, lut, ytox, ytob, misread=None, in_err=None):
    """Noise synthesis on image-sized planes xyb [3][ys][xs]: (planes, bar, raw bit patterns)."""
    _, ys, xs = np.shape(xyb)
    bits = noise_random(xs, ys, seed0, seed1, misread)
    out, bar = noise_add(xyb, bits.view(np.float32), lut, ytox, ytob, misread, in_err)
    return out, bar, bits


def features(xyb, n, kernels, out_xs, out_ys, seed0, seed1, lut, ytox, ytob, misread=None):
    """The order of dec_cache.cc:198-219 on frame-sized planes xyb [3][ys][xs]: upsampling by n, then noise at the image's
    resolution with the image's 256 x 256 squares. -> (planes [3][out_ys][out_xs], bar)."""
    if misread == "noise_before_upsampling":
        noisy = noise(xyb, seed0, seed1, lut, ytox, ytob)[0]
        ups = [upsample(noisy[c], n, kernels, out_xs, out_ys) for c in range(3)]
        return np.stack([u[0] for u in ups]), np.stack([upsample_bar(*u) for u in ups])
    ups = [upsample(xyb[c], n, kernels, out_xs, out_ys, misread) for c in range(3)]
    up = np.stack([u[0] for u in ups])
    out, bar, _ = noise(up, seed0, seed1, lut, ytox, ytob, misread, in_err=np.stack([upsample_bar(*u) for u in ups]))
    return out, bar


# ---- the cases both test files run (the reference of each is computed once: functools caches below)
UPSAMPLE_SIZES = ((1, 1), (2, 1), (1, 3), (3, 2), (5, 4), (63, 5), (64, 4), (65, 9), (130, 7))
NOISE_SIZES = ((1, 1), (2, 3), (15, 2), (16, 2), (17, 2), (32, 1), (33, 3), (256, 2), (257, 3), (272, 258), (513, 5))
NOISE_SEEDS = ((0, 0), (1, 0), (3, 7))
LUT_RAMP = tuple(np.float32(v) for v in (0.05, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 0.95))
LUT_WITH_ZERO = tuple(np.float32(v) for v in (0.6, 0.0, 0.5, 0.25, 0.75, 0.125, 1.0, 0.375))
STEP_AMPLITUDE = 1.0  # against Gaussian noise of sigma 0.05: the clamp bites on 18 % of the step planes' outputs


def coded_weights(n, seed=5):
    """A coded weight set for the synthetic cases: the default one, perturbed (the kernels still sum to about 1)."""
    rng = np.random.default_rng(1000 * n + seed)
    w = default_weights(n)
    return (w + rng.normal(0, 0.02, w.shape)).astype(np.float32)


def upsample_plane_case(xs, ys, content, seed=0):
    """The synthetic planes: 'noise' = Gaussian, 'step' = Gaussian + a step edge across the middle, 'constant'."""
    rng = np.random.default_rng(xs * 1009 + ys * 31 + seed)
    if content == "constant":
        return np.full((ys, xs), np.float32(0.3137), np.float32)
    p = rng.normal(0.4, 0.05, (ys, xs))
    if content == "step":
        yy, xx = np.mgrid[0:ys, 0:xs]
        p = p + STEP_AMPLITUDE * ((xx * 2 + yy) > (xs + ys / 2 - 1))
    return p.astype(np.float32)


def out_sizes(xs, ys, n):
    """The full size and the most ragged one."""
    return ((xs * n, ys * n), ((xs - 1) * n + 1, (ys - 1) * n + 1))


def noise_planes_case(xs, ys, seed=0):
    """X, Y, B planes whose strength inputs (Y -+ X) / 2 span below 0, [0, 7 / 6) and beyond."""
    rng = np.random.default_rng(xs * 7919 + ys * 13 + seed)
    y = rng.uniform(-0.2, 2.8, (ys, xs))
    x = rng.uniform(-0.3, 0.3, (ys, xs))
    b = rng.uniform(0.0, 1.0, (ys, xs))
    return np.stack([x, y, b]).astype(np.float32)
