"""The HIP spline kernel (-m gpu) against tests/splines_f64.py, the reading of splines.cc that shares no code with the
kernel, the host or the oracle. The bars are derived and recorded there.
A: k_splines_add through jxlhip_debug_splines on the host's own draw caches of test_splines_f64.CASES, over non-zero
   planes, against render() on the same segment list: the a-priori float32 bound.
B: the same on the crafted cache of test_splines_f64.crafted_rows (planes of 600 x 8, three strides of 256 columns): a span
   that starts at x = 300; one of 401 columns; spans clipped at x = 0 and at xsize; spans that end at -1 or start at xsize
   (nothing); span ends at exact ties (8.5 -> 9: x = 8 untouched; 20.5 -> 21; 0.5 - 2^-25 -> 0); negative 1 / sigma and
   negative sigma / 4 * intensity; forty segments over one sample; a row with none; row lists that are not ascending and name a
   segment twice; a band of rows, the others bit-identical to the input.
C: a lossless frame of zeros with curved strokes through JxlDecoder (f32 x 3) against dictionary -> reading -> samples.
D: a VarDCT frame with a coded base colour correlation: the device's own planes before the spline stage (the same frame
   coded without splines) in, its planes after it out.
C and D are held to 4 x the reading's own float32-to-float64 distance (END_TO_END_DISTANCE)."""
import ctypes

import numpy as np
import pytest

import replay_util as R
import splines_f64 as S
import test_splines_f64 as TS

pytestmark = pytest.mark.gpu

INVALID = 1  # JXLHIP_ERR_INVALID_ARGUMENT
F32 = np.float32


class Splines(ctypes.Structure):  # JxlHipSplines, include/jxl_amd_hip.h
    _fields_ = [("num_segments", ctypes.c_uint32), ("num_row_segments", ctypes.c_uint32), ("segments", ctypes.c_void_p),
                ("row_start", ctypes.c_void_p), ("row_segments", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def ctx(built):
    c = built.HipContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib(built):
    L = built.lib()
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.jxlhip_debug_splines.argtypes = [vp, vp, u32, u32, ctypes.POINTER(Splines), u32, u32, vp]
    return L


def _draw(lib, ctx, planes, segments, row_start, row_segments, band=None, expect=0):
    planes = np.ascontiguousarray(planes, F32)
    ys, xs = planes.shape[1:]
    seg = np.ascontiguousarray(segments, F32)
    rs, rl = np.ascontiguousarray(row_start, np.uint32), np.ascontiguousarray(row_segments, np.uint32)
    sp = Splines(len(seg), len(rl), seg.ctypes.data, rs.ctypes.data, rl.ctypes.data if len(rl) else None)
    out = np.full(planes.shape, 7.0, F32)
    y0, y1 = band or (0, ys)
    r = lib.jxlhip_debug_splines(ctx._h, planes.ctypes.data, xs, ys, ctypes.byref(sp), y0, y1, out.ctypes.data)
    assert r == expect, r
    return out


def _within(got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    bar = bound + S.U * np.abs(want)  # (the reading is float64: the result's own rounding to float32)
    return float((err / np.maximum(bar, 1e-300)).max())


@pytest.mark.parametrize("name", [n for n in TS.CASES if n != "single_point"])
def test_kernel_on_the_host_s_draw_caches(built, lib, ctx, name):
    J = built
    kind = TS.CASES[name][2]
    f = (J.ModFrame if kind == "lossless" else J.Frame)(TS.encode(J, name))
    c = f.splines()
    f.close()
    rng = np.random.default_rng(7)
    planes = rng.uniform(-1.0, 1.0, (3, c["ysize"], c["xsize"])).astype(F32)
    got = _draw(lib, ctx, planes, c["segments"], c["row_start"], c["row_segments"])
    want, bound = S.render(planes, c["segments"], c["row_start"], c["row_segments"])
    d = _within(got, want, bound)
    print(name, "largest distance / bar %.3f" % d)
    assert d <= 1 and np.abs(want - planes).max() > 0.05


def test_kernel_on_crafted_rows(lib, ctx):
    planes, segments, row_start, row_segments = TS.crafted_rows()
    got = _draw(lib, ctx, planes, segments, row_start, row_segments)
    want, bound = S.render(planes, segments, row_start, row_segments)
    d = _within(got, want, bound)
    print("crafted rows: largest distance / bar %.3f" % d)
    assert d <= 1
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    untouched = want == planes  # (no span covers the sample: the reading left it as given)
    assert untouched[:, 6].all() and untouched[:, 3, :9].all() and not untouched[:, 3, 9].any()  # the empty row; the tie at 8.5
    assert not untouched[:, 4, 0].any() and untouched[:, 4, 2:21].all() and not untouched[:, 4, 21].any()  # 0.5 - 2^-25 -> 0; 20.5 -> 21
    assert untouched[:, 0, :100].all() and not untouched[:, 0, 100].any() and not untouched[:, 0, 500].any() and untouched[:, 0, 501:].all()
    assert not untouched[:, 2, 0].any() and not untouched[:, 2, 599].any()  # clipped at both edges
    assert np.array_equal(bits(got)[untouched], bits(planes)[untouched])
    # a band: the rows outside come back bit for bit, the rows inside as in the whole run
    band = _draw(lib, ctx, planes, segments, row_start, row_segments, band=(2, 6))
    assert np.array_equal(bits(band[:, 2:6]), bits(got[:, 2:6]))
    assert np.array_equal(bits(band[:, :2]), bits(planes[:, :2])) and np.array_equal(bits(band[:, 6:]), bits(planes[:, 6:]))


def test_splines_entry_refuses_bad_arguments(lib, ctx):
    planes, segments, row_start, row_segments = TS.crafted_rows()
    out = np.full(planes.shape, 7.0, F32)
    p, o = planes.ctypes.data, out.ctypes.data
    keep = []

    def cache(seg=segments, rs=row_start, rl=row_segments, n=None):
        seg, rs, rl = np.ascontiguousarray(seg, F32), np.ascontiguousarray(rs, np.uint32), np.ascontiguousarray(rl, np.uint32)
        keep.extend([seg, rs, rl])
        return Splines(len(seg) if n is None else n, len(rl), seg.ctypes.data, rs.ctypes.data, rl.ctypes.data)

    good = cache()
    call = lambda h=ctx._h, pl=p, xs=600, ys=8, sp=good, y0=0, y1=8, ou=o: lib.jxlhip_debug_splines(h, pl, xs, ys, None if sp is None else ctypes.byref(sp), y0, y1, ou)
    assert call(h=None) == INVALID and call(pl=None) == INVALID and call(ou=None) == INVALID and call(sp=None) == INVALID
    assert call(xs=0) == INVALID and call(ys=0) == INVALID and call(xs=1 << 15) == INVALID
    assert call(y0=3, y1=3) == INVALID and call(y0=4, y1=3) == INVALID and call(y1=9) == INVALID
    assert call(sp=cache(n=0)) == INVALID                                    # an empty cache
    no_tables = Splines(len(segments), len(row_segments), None, None, None)
    assert call(sp=no_tables) == INVALID
    names_missing = row_segments.copy()
    names_missing[5] = len(segments)
    assert call(sp=cache(rl=names_missing)) == INVALID                       # a row list that names a missing segment
    descending = row_start.copy()
    descending[3] = descending[2] - 1
    assert call(sp=cache(rs=descending)) == INVALID
    short = row_start.copy()
    short[-1] -= 1
    assert call(sp=cache(rs=short)) == INVALID                               # the lists do not add up
    for col, v in ((0, np.nan), (2, np.inf), (3, np.inf), (4, np.nan), (6, -np.inf), (0, 2.0 ** 31), (2, 2.0 ** 31)):
        bad = segments.copy()
        bad[7, col] = v
        assert call(sp=cache(seg=bad)) == INVALID, (col, v)
    assert (out == 7.0).all()  # (nothing ran)
    assert call() == 0 and not (out == 7.0).any()


@pytest.mark.parametrize("name", [n for n in TS.END_TO_END_CASES if TS.CASES[n][2] == "lossless"])
def test_decoder_draws_what_the_reading_draws(built, tmp_path, name):
    """Case C. The planes of a lossless RGB frame of zeros are the spline stage's X, Y, B."""
    J = built
    splines, adjustment, kind = TS.CASES[name]
    rc, events, out, px = R.run(TS.encode(J, name), tmp_path, "f32", 3)
    assert rc == 0, out
    got = np.frombuffer(px, F32).reshape(TS.H, TS.W, 3).transpose(2, 0, 1)
    r = S.draw_cache(TS.dictionary_of(splines, adjustment), TS.W, TS.H, 0.0, 1.0)
    want, _ = S.render(np.zeros((3, TS.H, TS.W)), r["segments"], r["row_start"], r["row_segments"])
    d = float(np.abs(got - want).max())
    bar = S.DRAW_CACHE_MARGIN * S.END_TO_END_DISTANCE[name]
    print(name, "largest distance %.3g, bar %.3g" % (d, bar))
    assert d <= bar and np.abs(want).max() > 1


def _filtered_planes(J, data):
    f = J.Frame(data)
    c = J.HipContext()
    try:
        c.set_option("keep_filtered", 1)
        c.upload(f)
        c.run_all()
        c.sync()
        r, flags = c.errors()
        assert r == 0 and not any(flags)
        fi = c.frame_info
        return c.download("xyb_filtered")[:, :fi["ysize"], :fi["xsize"]].copy()
    finally:
        c.close()
        f.close()


def test_spline_stage_of_a_vardct_frame(built):
    """Case D. two_strokes_cmap: a VarDCT frame whose colour correlation bases are coded (0.25, 0.75). The same frame coded
    without its splines gives the device's planes before the stage; dictionary -> reading -> samples is added to them."""
    J = built
    name = "two_strokes_cmap"
    splines, adjustment, kind = TS.CASES[name]
    after = _filtered_planes(J, TS.encode(J, name))
    before = _filtered_planes(J, J.encode_rgb8(J.synth_image(TS.W, TS.H, seed=5), custom_cmap=1))
    assert after.shape == before.shape == (3, TS.H, TS.W)
    r = S.draw_cache(TS.dictionary_of(splines, adjustment), TS.W, TS.H, 0.25, 0.75)
    want, _ = S.render(before, r["segments"], r["row_start"], r["row_segments"])
    err = np.abs(after - want)
    bar = S.DRAW_CACHE_MARGIN * S.END_TO_END_DISTANCE[name] + 2 * S.U * np.abs(want)  # (+ the rounding of the sums onto the planes)
    print(name, "largest distance %.3g, bar %.3g" % (float(err.max()), S.DRAW_CACHE_MARGIN * S.END_TO_END_DISTANCE[name]))
    assert (err <= bar).all() and np.abs(want - before).max() > 0.05
