"""The host's spline code (jxh_splines.h) and the oracle's copy of it held to tests/splines_f64.py, the reading of
splines.cc that shares no code with either, without a GPU: FastCosf / FastErff as restated against cos / erf; the parsed
dictionary against what was written and, for the stream libjxl made (tests/golden/ref_wasm_splines.jxl), against the
integers committed in tests/golden/ref_wasm_splines_dictionary.json; both draw caches against the reading's, field by
field; the oracle's rendering against the reading's on the oracle's own cache; every misreading. The bars are derived and
recorded in splines_f64.py. The kernel's half is tests/test_gpu_splines_f64.py."""
import json
import math
import os

import numpy as np
import pytest

import splines_f64 as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "ref_wasm_splines.jxl")
F32 = np.float32

_FLAT = [[0] * 32, [300] + [0] * 31, [0] * 32]
_RICH = [[40, -6, 3] + [0] * 29, [300, 10, -25, 0, 7] + [0] * 27, [-50, 0, 12] + [0] * 29]


def _stroke(points, color=_FLAT, sigma=(9,)):
    return dict(points=list(points), color=[list(c) for c in color], sigma=list(sigma) + [0] * (32 - len(sigma)))


# name -> (splines as J.set_splines takes them, quantisation adjustment, kind of frame). Frames are 300 x 200.
CASES = {
    "line_220": ([_stroke([(40, 60), (260, 60)])], 0, "lossless"),
    "line_60_down": ([_stroke([(150, 40), (150, 100)], _RICH, (6, 2))], 0, "lossless"),
    "one_pixel": ([_stroke([(100, 100), (101, 100)])], 0, "lossless"),
    "single_point": ([_stroke([(100, 100)])], 0, "lossless"),
    "diagonal": ([_stroke([(30, 30), (150, 150)], _RICH, (10, -3, 1))], 5, "lossless"),
    "four_point_curve": ([_stroke([(20, 30), (120, 90), (220, 40), (280, 160)], [[40] + [0] * 31, [300, 10] + [0] * 30, [0] * 32], (12,))], -3,
                         "lossless"),
    "two_point_stroke": ([_stroke([(50, 180), (150, 120)], [[0] * 32, [-200] + [0] * 31, [100] + [0] * 31], (6, 2))], -3, "lossless"),
    "hairpin": ([_stroke([(30, 30), (200, 40), (35, 50)], _RICH, (7, 0, 2))], 5, "lossless"),
    "closed_loop": ([_stroke([(100, 50), (180, 80), (150, 150), (70, 140), (100, 50)], _RICH, (8, 1))], 0, "lossless"),
    "across_the_frame": ([_stroke([(340, 100), (-40, 100)], _RICH, (9, 2))], 0, "lossless"),
    "sigma_changes_sign": ([_stroke([(40, 120), (150, 70), (260, 130)], _RICH, (1, 8))], 0, "lossless"),
    "two_strokes_vardct": ([_stroke([(20, 30), (120, 90), (220, 40), (280, 160)], _RICH, (12, 3)),
                            _stroke([(50, 180), (150, 120)], [[0] * 32, [-200, 30] + [0] * 30, [100] + [0] * 31], (6, 2))], -3, "vardct"),
    "two_strokes_cmap": ([_stroke([(20, 30), (120, 90), (220, 40), (280, 160)], _RICH, (12, 3)),
                          _stroke([(50, 180), (150, 120)], [[0] * 32, [-200, 30] + [0] * 30, [100] + [0] * 31], (6, 2))], 5, "vardct_cmap"),
    "upsampled_frame": ([_stroke([(10, 15), (60, 45), (110, 20)], _RICH, (12, 3))], 0, "vardct_upsampled2"),
}
W, H = 300, 200
FIELDS = ("centre", "maximum_distance", "inv_sigma", "sigma_over_4_times_intensity", "colour")
COLUMNS = {"centre": [0, 1], "maximum_distance": [2], "inv_sigma": [3], "sigma_over_4_times_intensity": [4], "colour": [5, 6, 7]}


def dictionary_of(splines, adjustment):
    """What J.set_splines takes -> what splines_f64.draw_cache takes (splines.cc:396-408: double deltas)."""
    out = []
    for sp in splines:
        p = np.asarray(sp["points"], np.int64).reshape(-1, 2)
        steps = np.diff(p, axis=0)
        deltas = np.diff(np.concatenate([np.zeros((1, 2), np.int64), steps]), axis=0)
        out.append(dict(start=tuple(int(v) for v in p[0]), deltas=[tuple(int(v) for v in d) for d in deltas],
                        color=[list(c) for c in sp["color"]], sigma=list(sp["sigma"])))
    return dict(adjustment=adjustment, splines=out)


def encode(J, name):
    splines, adjustment, kind = CASES[name]
    J.set_splines(splines, quantization_adjustment=adjustment)
    try:
        if kind == "lossless":
            return J.encode_lossless(np.zeros((H, W, 3), np.uint8))
        kw = {"vardct": {}, "vardct_cmap": dict(custom_cmap=1), "vardct_upsampled2": dict(upsampling=2)}[kind]
        return J.encode_rgb8(J.synth_image(W, H, seed=5), **kw)
    finally:
        J.set_splines(None)


def spans_of(row_start, row_segments, n):
    """[n][2]: the first row that lists each segment and one past the last (rows in between checked to list it too)."""
    first, count = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    last = np.full(n, -1, np.int64)
    for y in range(len(row_start) - 1):
        l = row_segments[row_start[y]:row_start[y + 1]].astype(np.int64)
        assert (np.diff(l) > 0).all(), "row %d does not list its segments in order" % y
        first[l[first[l] < 0]] = y
        last[l] = y
        count[l] += 1
    assert (count == last - first + 1)[first >= 0].all()
    return np.stack([first, last + 1], axis=1)


def measured_distance(r32, r64):
    return {f: float(np.abs(r32["segments"][:, COLUMNS[f]].astype(np.float64) - r64["segments"][:, COLUMNS[f]]).max(initial=0.0)) for f in FIELDS}


def ambiguous_ends(reading, bar):
    """Which span ends the bar cannot tell: the llround argument is within it of a half-integer."""
    a = np.asarray(reading["span_args"], np.float64)
    return np.abs(np.abs(a - np.floor(a)) - 0.5) <= bar


def compare_cache(name, what, segments, row_start, row_segments, r64, distance):
    """A draw cache (host's or oracle's) against the reading: the same points and segments, every field within 4 x the
    reading's own float32 distance for the case, row spans equal wherever the reading's rounding is not a near-tie."""
    n = len(r64["segments"])
    assert len(segments) == n, (name, what, len(segments), n)
    report = {}
    for f in FIELDS:
        bar = S.DRAW_CACHE_MARGIN * distance[f]
        d = float(np.abs(segments[:, COLUMNS[f]].astype(np.float64) - r64["segments"][:, COLUMNS[f]]).max(initial=0.0))
        report[f] = (d, bar)
        assert d <= bar, (name, what, f, d, bar)
    if n:
        spans = spans_of(row_start, row_segments, n)
        bar = S.DRAW_CACHE_MARGIN * max(distance["centre"], distance["maximum_distance"]) * 2
        loose = ambiguous_ends(r64, bar)
        assert loose.mean() <= 0.01, (name, what, float(loose.mean()))
        visible = r64["spans"][:, 0] < r64["spans"][:, 1]
        diff = spans - r64["spans"]
        assert (diff[~loose] == 0).all() and (np.abs(diff) <= 1).all() and visible.all(), (name, what, diff[np.any(diff != 0, axis=1)][:4])
    else:
        assert int(row_start[-1]) == 0
    return report


@pytest.fixture(scope="module")
def readings():
    """name -> (frame size, y_to_x, y_to_b, float32 reading, float64 reading)."""
    out = {}
    for name, (splines, adjustment, kind) in CASES.items():
        xs, ys = (150, 100) if kind == "vardct_upsampled2" else (W, H)
        ytox, ytob = (0.25, 0.75) if kind == "vardct_cmap" else (0.0, 1.0)
        d = dictionary_of(splines, adjustment)
        out[name] = (xs, ys, ytox, ytob, S.draw_cache(d, xs, ys, ytox, ytob, F32), S.draw_cache(d, xs, ys, ytox, ytob, np.float64))
    return out


def test_fast_math_restatements_are_within_the_reference_bounds():
    """fast_math-inl.h states 7e-5 for FastCosf (fast_math_test.cc) and 7e-4 for FastErff. The splines call the first with
    pi / 32 * i * (31 progress + 1 / 2), i <= 31: [0, 96]; the second with (d / 2 +- 2^-1.5) / sigma: any real, and flat
    beyond +-6."""
    x = np.linspace(0.0, 96.0, 960001)
    for T in (np.float64, F32):
        assert np.abs(S.fast_cos(x, T) - np.cos(x)).max() < 7e-5
    x = np.concatenate([np.linspace(-8.0, 8.0, 160001), np.geomspace(8.0, 1e6, 2001), -np.geomspace(8.0, 1e6, 2001)])
    erf = np.array([math.erf(v) for v in x])
    for T in (np.float64, F32):
        assert np.abs(S.fast_erf(x, T) - erf).max() < 7e-4
    assert float(S.fast_erf(0.0)) == 0.0 and float(S.fast_cos(0.0)) == pytest.approx(1.0, abs=7e-5)


def test_reading_float32_against_float64(readings):
    """The reading against itself: the same points and segments in both precisions, at most 1 % of the span ends near a tie,
    and the distances the draw-cache bars are made of. They are printed; splines_f64.DRAW_CACHE_DISTANCE holds them."""
    measured = {}
    for name, (xs, ys, ytox, ytob, r32, r64) in readings.items():
        assert r32["points"] == r64["points"], name
        extra = len(r32["segments"]) - len(r64["segments"])
        assert extra == 0, (name, extra)
        measured[name] = measured_distance(r32, r64)
        if len(r64["segments"]):
            bar = S.DRAW_CACHE_MARGIN * max(measured[name]["centre"], measured[name]["maximum_distance"]) * 2
            loose = ambiguous_ends(r64, bar)
            diff = r32["spans"] - r64["spans"]
            assert loose.mean() <= 0.01 and (diff[~loose] == 0).all(), (name, float(loose.mean()))
    print("DRAW_CACHE_DISTANCE = {")
    for name in CASES:
        print("    %r: {%s}," % (name, ", ".join("%r: %.3g" % (f, measured[name][f]) for f in FIELDS)))
    print("}")
    assert set(S.DRAW_CACHE_DISTANCE) == set(CASES)
    for name in CASES:
        for f in FIELDS:
            m, c = measured[name][f], S.DRAW_CACHE_DISTANCE[name][f]
            assert (m == 0 and c == 0) or 0.75 * c <= m <= 1.25 * c, (name, f, m, c)


END_TO_END_CASES = ("four_point_curve", "hairpin", "closed_loop", "sigma_changes_sign", "two_strokes_cmap")


def test_reading_end_to_end_float32_against_float64(readings):
    """Dictionary -> samples in both precisions, on planes of zeros: what the end-to-end bars are made of (printed;
    splines_f64.END_TO_END_DISTANCE holds them)."""
    measured = {}
    for name in END_TO_END_CASES:
        xs, ys, ytox, ytob, r32, r64 = readings[name]
        zeros = np.zeros((3, ys, xs))
        p32, _ = S.render(zeros, r32["segments"], r32["row_start"], r32["row_segments"], dtype=F32)
        p64, _ = S.render(zeros, r64["segments"], r64["row_start"], r64["row_segments"])
        measured[name] = float(np.abs(p32.astype(np.float64) - p64).max())
    print("END_TO_END_DISTANCE = {%s}" % ", ".join("%r: %.3g" % kv for kv in measured.items()))
    assert set(S.END_TO_END_DISTANCE) == set(END_TO_END_CASES)
    for name, m in measured.items():
        assert 0.75 * S.END_TO_END_DISTANCE[name] <= m <= 1.25 * S.END_TO_END_DISTANCE[name], (name, m)


def test_a_single_control_point_draws_nothing(built, readings):
    """splines.cc:303-306, 707-713: one point, twice (as the first point and as the last, which closes a step of length 0):
    arc length 0, no segment."""
    xs, ys, ytox, ytob, r32, r64 = readings["single_point"]
    assert r64["points"] == [2] and len(r64["segments"]) == 0 and int(r64["row_start"][-1]) == 0
    J = built
    f = J.ModFrame(encode(J, "single_point"))
    got = f.splines()
    f.close()
    assert got is not None and got["segments"].shape == (0, 8) and not got["row_start"].any() and len(got["row_start"]) == H + 1


@pytest.fixture(scope="module")
def caches(built):
    """name -> (stream, the host's Frame / ModFrame.splines(), the oracle's dump, the oracle's planes)."""
    import jxlo
    J = built
    out = {}
    for name, (splines, adjustment, kind) in CASES.items():
        data = encode(J, name)
        f = (J.ModFrame if kind == "lossless" else J.Frame)(data)
        host = f.splines()
        f.close()
        o = jxlo.Decoded(data)
        seg = o.buffer("spline_segments")
        oracle = dict(segments=np.zeros((0, 8), F32) if seg is None else seg.reshape(-1, 8), row_start=o.buffer("spline_row_start"),
                      row_segments=o.buffer("spline_row_segments"), used=o.buffer("spline_used"))
        if oracle["row_segments"] is None:
            oracle["row_segments"] = np.zeros(0, np.uint32)
        planes = o.planes("rgbf").copy() if kind == "lossless" else None
        o.close()
        out[name] = (data, host, oracle, planes)
    return out


def test_host_dictionary_is_what_was_written(built, caches):
    for name, (splines, adjustment, kind) in CASES.items():
        host = caches[name][1]
        assert host["dictionary"] == dictionary_of(splines, adjustment), name
        xs, ys = (150, 100) if kind == "vardct_upsampled2" else (W, H)  # (an upsampled frame's cache: at the frame's own size)
        want = (xs, ys, 0.25, 0.75) if kind == "vardct_cmap" else (xs, ys, 0.0, 1.0)
        assert (host["xsize"], host["ysize"], host["y_to_x"], host["y_to_b"]) == want, name
        assert tuple(caches[name][2]["used"]) == (want[2], want[3], xs, ys), name
    assert built.ModFrame(built.encode_lossless(np.zeros((8, 8, 3), np.uint8))).splines() is None


def test_reference_stream_dictionary_is_the_committed_one(built):
    """One stroke: a start, a few control points, colour and sigma integers: tests/golden/ref_wasm_splines_dictionary.json
    holds the integers (reviewed against the stream's purpose, jxl_from_tree's one spline)."""
    f = built.ModFrame(open(REF, "rb").read())
    got = f.splines()
    f.close()
    want = json.load(open(os.path.join(GOLDEN, "ref_wasm_splines_dictionary.json")))
    have = json.loads(json.dumps(got["dictionary"]))  # (tuples as lists)
    assert have == want
    assert len(want["splines"]) == 1 and (got["xsize"], got["ysize"], got["y_to_x"], got["y_to_b"]) == (320, 320, 0.0, 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_host_and_oracle_draw_caches_against_the_reading(caches, readings, name):
    xs, ys, ytox, ytob, r32, r64 = readings[name]
    data, host, oracle, planes = caches[name]
    distance = S.DRAW_CACHE_DISTANCE[name]
    for what, c in (("host", host), ("oracle", oracle)):
        assert len(c["row_start"]) == ys + 1
        rep = compare_cache(name, what, c["segments"], c["row_start"], c["row_segments"], r64, distance)
        print(name, what, {f: "%.2g / %.2g" % v for f, v in rep.items()})


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[2] == "lossless" and n != "single_point"])
def test_oracle_rendering_on_its_own_cache(caches, name):
    """A lossless frame of zeros: the oracle's planes are its spline stage's output. Held to render() on the oracle's own
    segment list, within the a-priori float32 bound."""
    data, host, oracle, planes = caches[name]
    want, bound = S.render(np.zeros((3, H, W)), oracle["segments"], oracle["row_start"], oracle["row_segments"])
    err = np.abs(planes.astype(np.float64) - want)
    bar = bound + S.U * np.abs(want)
    print(name, "largest distance / bar %.3f" % float((err / np.maximum(bar, 1e-300)).max()), "largest sample %.3g" % float(np.abs(want).max()))
    assert (err <= bar).all() and np.abs(want).max() > 0.05


def _cache_moves(right, wrong, distance):
    """Whether a misread draw cache differs from the reading by more than ten bars somewhere (or in a count)."""
    if right["points"] != wrong["points"] or len(right["segments"]) != len(wrong["segments"]):
        return True
    for f in FIELDS:
        d = np.abs(right["segments"][:, COLUMNS[f]] - wrong["segments"][:, COLUMNS[f]]).max(initial=0.0)
        if d > 10 * S.DRAW_CACHE_MARGIN * distance[f] and d > 0:
            return True
    return False


def test_every_geometry_misreading_shows(readings):
    shown = {}
    for m in S.GEOMETRY_MISREADINGS:
        for name, (splines, adjustment, kind) in CASES.items():
            xs, ys, ytox, ytob, r32, r64 = readings[name]
            wrong = S.draw_cache(dictionary_of(splines, adjustment), xs, ys, ytox, ytob, np.float64, misread=m)
            if _cache_moves(r64, wrong, S.DRAW_CACHE_DISTANCE[name]):
                shown.setdefault(m, []).append(name)
        print(m, "shows on", shown.get(m, []))
    assert set(shown) == set(S.GEOMETRY_MISREADINGS), set(S.GEOMETRY_MISREADINGS) - set(shown)


def crafted_rows():
    """The crafted draw cache of tests/test_gpu_splines_f64.py (its docstring lists what is in it): planes of 600 x 8."""
    seg = lambda cx, cy, maxd, inv_sigma, s4i, col=(0.5, -0.25, 1.0): [cx, cy, maxd, inv_sigma, s4i] + list(col)
    segments = [
        seg(400.25, 0.5, 100.0, 0.05, 0.7),                 # 0: columns 300 .. 500: starts in the second stride
        seg(300.0, 1.0, 200.0, 0.02, 0.4),                  # 1: 100 .. 500: 401 columns, two trips of a thread
        seg(3.0, 2.0, 40.0, 0.08, 0.5),                     # 2: clipped at x = 0
        seg(590.0, 2.0, 30.0, 0.1, 0.6),                    # 3: clipped at x = xsize
        seg(-3.0, 3.0, 2.0, 0.5, 0.9),                      # 4: end == -1: nothing
        seg(603.0, 3.0, 3.0, 0.5, 0.9),                     # 5: start == xsize: nothing
        seg(20.75, 3.0, 12.25, 0.09, 0.8),                  # 6: 20.75 - 12.25 = 8.5 -> 9 (x = 8 untouched); 20.75 + 12.25 = 33
        seg(50.25, 3.5, 29.75, 0.11, 0.8),                  # 7: 50.25 + 29.75 = 80: no tie; 50.25 - 29.75 = 20.5 -> 21
        seg(0.75, 4.0, 0.25 + 2.0 ** -25, 0.06, 0.8),       # 8: 0.75 - maxd = 0.5 - 2^-25 -> 0; the sum with 0.5 rounds to 1
        seg(130.5, 4.5, 60.0, -0.07, 0.5),                  # 9: negative inv_sigma
        seg(450.0, 4.0, 70.0, 0.05, -0.6),                  # 10: negative sigma / 4 * intensity
        seg(100.5, 20.5, 80.0, 0.04, 0.3),                  # 11: far above the rows it is drawn on
    ]
    segments += [seg(250.0 + 0.37 * k, 5.0 + 0.01 * k, 9.0 + 0.5 * k, 0.2 - 0.002 * k, 0.1 + 0.01 * k, (0.3 - 0.02 * k, 0.1, -0.2 + 0.01 * k))
                 for k in range(40)]                        # 12 .. 51: forty over the samples around x = 257
    rows = [[0, 1], [1, 0, 11], [2, 3, 1], [4, 5, 6, 7], [8, 9, 10, 7], list(range(12, 52)), [], [11, 51, 12, 3]]
    row_start = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    row_segments = np.array([i for r in rows for i in r], np.uint32)
    rng = np.random.default_rng(5)
    planes = rng.uniform(-1.0, 1.0, (3, 8, 600)).astype(F32)
    return planes, np.array(segments, F32), row_start, row_segments


def test_every_rendering_misreading_shows():
    planes, segments, row_start, row_segments = crafted_rows()
    right, bound = S.render(planes, segments, row_start, row_segments)
    # the ties: x = 8 of row 3 is not drawn on by segment 6 (llround(8.5) = 9) and x = 21 is the first of segment 7
    only6, _ = S.render(np.zeros_like(planes), segments[6:7], np.array([0, 0, 0, 0, 1, 1, 1, 1, 1], np.uint32), np.array([0], np.uint32))
    assert not only6[:, 3, :9].any() and only6[:, 3, 9].all() and only6[:, 3, 33].all() and not only6[:, 3, 34:].any()
    shown = {}
    for m in S.RENDER_MISREADINGS:
        wrong, _ = S.render(planes, segments, row_start, row_segments, misread=m)
        moved = np.abs(wrong - right) > 10 * (bound + S.U * np.abs(right))
        shown[m] = sorted(set(int(y) for y in np.nonzero(moved)[1]))
        print(m, "shows on rows", shown[m])
    assert all(shown[m] for m in S.RENDER_MISREADINGS), shown
    assert 3 in shown["tie_half_even"] and shown["tie_floor_plus_half"] == [4]


def test_spline_accessors_under_sanitizers(built, tmp_path):
    """tests/c/splines_kats.cc: jxlamd_frame_splines / jxlamd_modframe_splines built with AddressSanitizer + UBSan around
    libjxl_amd/csrc/api/jxl_api.cc, as a program of its own: sized copies into blocks of exactly the size given (the whole, one
    byte less, 3 bytes, none), then the draw cache walked the way the kernel walks it."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    J = built
    out = os.path.join(str(tmp_path), "splines_kats")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-Wno-unused-function", "-Wno-subobject-linkage", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "splines_kats.cc"), "-o", out, "-lpthread"], check=True)
    for kind, names in (("modular", ["four_point_curve", "single_point", "across_the_frame"]), ("vardct", ["two_strokes_cmap", "upsampled_frame"])):
        paths = []
        for name in names:
            paths.append(os.path.join(str(tmp_path), name + ".jxl"))
            open(paths[-1], "wb").write(encode(J, name))
        if kind == "modular":
            paths += [REF, os.path.join(str(tmp_path), "plain.jxl")]
            open(paths[-1], "wb").write(J.encode_lossless(np.zeros((8, 8, 3), np.uint8)))
        r = subprocess.run([out, kind] + paths, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(paths) and sum("segments:" in l for l in lines) == len(names) + (kind == "modular"), r.stdout
        if kind == "modular":  # (a frame without splines; a single control point: a dictionary, no segment)
            assert "no splines" in lines[-1] and "segments: 0 " in lines[1], r.stdout
