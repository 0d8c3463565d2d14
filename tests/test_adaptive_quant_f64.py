"""The reference's initial adaptive quant field as the CPU stream writer states it (adaptive_quant=1: the stand-alone
double jxlenc_cpu_initial_quant_field, the model of enc_forward_model with no context, and the streams of encode_rgb8)
against the float64 reading of tests/adaptive_quant_f64.py, which shares no code with it. This is where RTOL and
QF_DELTA_MEASURED of that file were measured: run with -s, every test prints its figures before it asserts."""
import functools

import numpy as np
import pytest

import adaptive_quant_f64 as A
import enc_fwd_f64 as E

# (size, kw): the whole-path cases. The image of a case is synth_image(seed = width + 11), as in test_enc_fwd_f64.py, but for
# 1000x700, whose seed is 1014: at distance 0.3 the Y DC of that frame is 1000 .. 1200 quantisation steps, where half a
# float32 ulp (6e-5 steps) is more than enc_fwd_f64.DELTA['dc'] (5e-5), and with seeds 1011 .. 1013 one or two of the 99000
# values lie between the two from a rounding boundary (1011: 1163.49994, whose nearest float32 is 1163.5). Judged by the
# reading alone, seed 1014 has no DC value outside DELTA['dc'] that lies within three float32 ulps of a boundary.
SEEDS = {(1000, 700): 1014}
CASES = [((8, 8), dict(distance=0.3, gab=0)), ((113, 4), dict(distance=1.0, strategy_mode=0)), ((263, 9), dict(distance=4.0)),
         ((257, 260), dict(distance=1.0, gab=0)), ((520, 300), dict(distance=1.0)), ((520, 300), dict(distance=4.0, gab=0)),
         ((1000, 700), dict(distance=0.3))]
MOSAIC_KW = dict(distance=1.0, gab=0, strategy_mode=1)


@functools.lru_cache(maxsize=None)
def planes(kind, size):
    p = A.crafted(kind, size[0], size[1])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reading(kind, size, distance):
    aq, mask = A.initial_quant_field(planes(kind, size), distance)
    aq.setflags(write=False)
    mask.setflags(write=False)
    return aq, mask


def check_entry(J, ctx, kind):
    """One plane kind over every size and distance: aq_map and mask of the stand-alone entry (the device's on `ctx`, the
    CPU double's without) within RTOL of the reading, relative. Returns the largest deviations."""
    worst = [0.0, 0.0]
    bad = []
    for size in A.SIZES:
        for d in A.DISTANCES:
            want = reading(kind, size, d)
            got = J.initial_quant_field(planes(kind, size), d, ctx=ctx)
            for i, name in enumerate(("aq_map", "mask")):
                assert got[i].shape == want[i].shape == (size[1] // 8, size[0] // 8)
                dev = float(np.max(np.abs(got[i] - want[i]) / np.abs(want[i])))
                worst[i] = max(worst[i], dev)
                if not dev <= A.RTOL:
                    bad.append((name, size, d, dev))
    print("%s: largest relative deviation aq_map %.3e mask %.3e (RTOL %.3e)" % (kind, worst[0], worst[1], A.RTOL))
    assert not bad, bad[:6]
    return worst


@pytest.mark.parametrize("kind", A.KINDS)
def test_cpu_entry_matches_float64_reading(built, kind):
    check_entry(built, None, kind)


def test_crafted_planes_reach_the_arms_they_are_for():
    """The planes do what their names say, judged by the reading alone: the blue plane has block sums below kMaxLimit
    kLimit, capped ones, and folded ones on either side of the cap; the negative plane drives the ratio's argument below
    zero; the steps plane reaches the 0.2 clamp; the distances sit on both sides of 2 and of the dampen ramp."""
    lim, kmax = 0.010474084867598155, 15.463398341612438
    x, y, b = (p.astype(np.float64) for p in planes("blue", (264, 264)))
    eff = A._blocks(y) + 0.0031994768654636393 + np.abs(A._blocks(x))
    s = np.where(A._blocks(b) > eff, np.minimum(A._blocks(b) - eff, lim), 0.0).sum(axis=(2, 3))
    folded = 64 * lim - s[s >= 32 * lim]
    assert (s < kmax * lim).any() and ((s >= kmax * lim) & (s < 32 * lim)).any()
    assert (folded >= kmax * lim).any() and (folded < kmax * lim).any()
    x, y, b = planes("negative", (72, 72))
    assert (y + 0.019 < 0).any() and (y + 0.16 - x < 0).any() and (y + 0.16 + x < 0).any() and (y + 0.16 + x > 0).any()
    y = planes("steps", (72, 72))[1].astype(np.float64)
    p = np.pad(y, 1, mode="edge")
    base = 0.25 * (p[2:, 1:-1] + p[:-2, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:])
    v = (A.ratio(y + 0.019, False) * (y - base)) ** 2
    assert (v > 0.2).any() and (v < 0.2).any()
    assert [A.dampen(d) for d in (1.9, 2.0, 8.0, 14.0, 15.0)] == [1.0, 1.0, 0.5, 0.0, 0.0]
    assert not np.allclose(A.erosion_weights(0.3), A.erosion_weights(1.9)) and np.allclose(A.erosion_weights(2.5), A.erosion_weights(4.0))


def test_entry_rejects_bad_arguments(built):
    J = built
    with pytest.raises(J.JxlAmdError):
        J.initial_quant_field(np.zeros((3, 12, 8), np.float32), 1.0)
    with pytest.raises(J.JxlAmdError):
        J.initial_quant_field(np.zeros((3, 8, 8), np.float32), 0.0)


# ---------------------------------------------------------------- the whole path
@functools.lru_cache(maxsize=None)
def aq_header(J, distance):
    """The quantiser fields an adaptive_quant=1 stream of this distance carries, as the oracle reads them; they are those
    of the reading's ComputeGlobalScaleAndQuant."""
    import jxlo
    o = jxlo.Decoded(J.encode_rgb8(J.synth_image(64, 64, seed=5), distance=distance, adaptive_quant=1), dumps=False)
    h = o.quant_header
    o.close()
    assert (h["global_scale"], h["quant_dc"]) == A.quantizer_scalars(distance), (h, A.quantizer_scalars(distance))
    return h


def qf_reading(R, img, acs, distance, gab):
    """The value before truncation of the integer field at the first blocks of `acs`."""
    xyb = E.opsin_xyb(img, R.xb * 8, R.yb * 8)
    aq, _ = A.initial_quant_field(xyb, distance if gab else 0.62 * distance)
    return A.adjust_quant_field(aq, acs, distance, E.COVERED) * R.inv_gs + 0.5


def check_forward_aq(model, img, header, distance=1.0, gab=1, strategy_mode=1, max_band=1e-3):
    """enc_fwd_f64.check_forward for an adaptive_quant=1 model: the transform choices as there; qf at first blocks by
    decide() under the model's own choices with delta = QF_DELTA_REL t, the ambiguous band at most 1 % of the first blocks; DC and AC
    with the existing reading under the model's qf and the mode's header scalars."""
    R = E.Reading(img, header, distance=distance, gab=gab, strategy_mode=strategy_mode)
    acs = model["acs"]
    assert acs.shape == R.acs.shape
    amb_tiles = np.repeat(np.repeat(R.act_margin <= E.DELTA["act"], 8, 0), 8, 1)[:R.yb, :R.xb]
    bad = (acs != R.acs) & ~amb_tiles
    assert not bad.any(), "transform choice differs from the reading at %d blocks" % bad.sum()
    n_amb_tiles = int((R.act_margin <= E.DELTA["act"]).sum())
    assert n_amb_tiles <= max(1, 0.01 * R.act_margin.size), n_amb_tiles
    first = (acs & 1) == 1
    t = qf_reading(R, img, acs, distance, gab)[first]
    got = model["qf"][first]
    differs = got != E.quant_field_int(t)
    margin = float(np.abs(t[differs] - np.rint(t[differs])).max()) if differs.any() else 0.0
    amb_q, wrong = E.decide(got, t, E.quant_field_int, A.QF_DELTA_REL * t)
    print("qf: %d first blocks, %d rounded differently (largest distance from the boundary %.3e), %d in the band of %.1e t (t up to %.1f)" % (
        first.sum(), differs.sum(), margin, amb_q.sum(), A.QF_DELTA_REL, t.max()))
    assert not wrong.any(), "quant field differs at %d first blocks: %s vs reading %s" % (wrong.sum(), got[wrong][:4], t[wrong][:4])
    assert amb_q.sum() <= 0.01 * first.sum(), (int(amb_q.sum()), int(first.sum()))
    assert len(np.unique(got)) > 1 or first.sum() == 1, "a constant field is not an adaptive one"
    dc, co, used = R.transform(acs, model["qf"], dc_y=model["dc"][1], coeffs_y=model["coeffs"][:, 1])
    amb_d, wrong = E.decide(model["dc"], dc, E.round_dc, E.DELTA["dc"])
    assert not wrong.any(), "DC differs at %d of %d" % (wrong.sum(), wrong.size)
    sel = np.broadcast_to(used[:, None, :], co.shape)
    amb_a, wrong = E.decide(model["coeffs"][sel], co[sel], E.quantise_ac, E.DELTA["ac"])
    assert not wrong.any(), "AC differs at %d of %d" % (wrong.sum(), wrong.size)
    assert amb_d.sum() <= max_band * dc.size and amb_a.sum() <= max_band * sel.sum(), (amb_d.sum(), amb_a.sum())
    return margin


def case_image(J, size):
    return J.synth_image(size[0], size[1], seed=SEEDS.get(size, size[0] + 11))


def _kw(kw):
    return dict(distance=kw.get("distance", 1.0), gab=kw.get("gab", 1), strategy_mode=kw.get("strategy_mode", 1))


@pytest.mark.parametrize("size,kw", CASES)
def test_forward_cpu_model_matches_float64_reading(built, size, kw):
    J = built
    img = case_image(J, size)
    model = J.enc_forward_model(img, None, adaptive_quant=1, **kw)
    check_forward_aq(model, img, aq_header(J, kw.get("distance", 1.0)), **_kw(kw))


def test_forward_cpu_model_mosaic_matches_float64_reading(built):
    J = built
    model = J.enc_forward_model(E.mosaic(), None, adaptive_quant=1, **MOSAIC_KW)
    assert len(np.unique(model["acs"][(model["acs"] & 1) == 1])) == 12  # every size class, so every aggregation
    check_forward_aq(model, E.mosaic(), aq_header(J, MOSAIC_KW["distance"]), **_kw(MOSAIC_KW))


def test_default_mode_is_untouched(built):
    J = built
    img = J.synth_image(200, 120, seed=4)
    assert J.encode_rgb8(img, adaptive_quant=0) == J.encode_rgb8(img)
    with pytest.raises(J.JxlAmdError):
        J.encode_rgb8(img, adaptive_quant=2)
    with pytest.raises(J.JxlAmdError):
        J.encode_rgb8(img, adaptive_quant=1, color_transform=2)


# ---------------------------------------------------------------- round trip
def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


@pytest.mark.parametrize("size,distance", [((200, 120), 1.0), ((200, 120), 4.0), ((520, 300), 1.0), ((520, 300), 4.0)])
def test_stream_round_trip(built, size, distance):
    import jxlo
    J = built
    img = J.synth_image(size[0], size[1], seed=21)
    data = J.encode_rgb8(img, distance=distance, adaptive_quant=1)
    back = jxlo.Decoded(data, dumps=False).rgb8
    assert back.shape == img.shape
    plain = jxlo.Decoded(J.encode_rgb8(img, distance=distance), dumps=False).rgb8
    print("%dx%d d%.1f: adaptive_quant=1 %d bytes %.2f dB; default %d bytes %.2f dB" % (
        size[0], size[1], distance, len(data), psnr(back, img), len(J.encode_rgb8(img, distance=distance)), psnr(plain, img)))
    t = {}
    assert J.encode_rgb8_hooks_cpu(img, timings=t, distance=distance, adaptive_quant=1) == data
    assert t["device_entropy"] > 0
