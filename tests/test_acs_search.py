"""The forward path with the reference's AC-strategy search (adaptive_quant=1, acs_search=1 the aligned walk, 2 with the
floating passes) as the CPU stream writer states it. The search is wired from parts that are each held to a reading of their
own elsewhere (mask1x1, the adaptive field, the cost estimate, the walk), so the checks here are about the wiring, and exact:
the call's own search data (enc_search_debug) must be what the stand-alone entries give on the call's own planes, and the
call's transform choices what the walk's reading gives on the call's own table. Then the quant field, DC and AC under the
call's own choices go through the existing float64 readings with their tolerances unchanged; mode 2 gives them transforms
that are not aligned to their own size. The check_* functions take the context so that tests/test_gpu_acs_search.py runs them
on the device. Run with -s for the figures."""
import numpy as np
import pytest

import acs_walk_np as W
import adaptive_quant_f64 as A
import enc_fwd_f64 as E
from test_adaptive_quant_f64 import aq_header, qf_reading

# (size, distance, gab): one tile; partial tiles in both directions; several tiles. gab is 0 for one of them.
CASES = (((64, 64), 1.0, 1), ((88, 104), 4.0, 0), ((200, 136), 1.0, 1))
MODES = (1, 2)


def case_image(J, size):
    return J.synth_image(size[0], size[1], seed=size[0] + 11)


def check_wiring(J, ctx, size, distance, gab, mode):
    """ctx: a HipContext or a CpuEncContext (both keep the last call's search data). Returns (model, search data)."""
    img = case_image(J, size)
    model = J.enc_forward_model(img, ctx, adaptive_quant=1, acs_search=mode, distance=distance, gab=gab)
    s = J.enc_search_debug(ctx)  # (before any stand-alone call: the device's aq_map buffer is shared with initial_quant_field)
    dev = None if isinstance(ctx, J.CpuEncContext) else ctx
    yb, xb = model["acs"].shape
    # the walk's reading on the call's own table gives the call's choices
    acs, _, asked, _ = W.walk_frame(s["estimates"], xb, yb, distance, mode - 1)
    assert np.array_equal(model["acs"], acs), "%d blocks differ from the walk on the call's own table" % (model["acs"] != acs).sum()
    assert W.valid_tiling(model["acs"])
    # the table is the stand-alone estimate on the call's own planes, field and masking with zero factors
    cand, index = J.acs_walk_candidates(xb, yb, mode - 1)
    tiles = s["estimates"].shape[0]
    est = J.estimate_entropy(s["after"], s["aq_map"], s["mask1x1"], np.zeros(tiles, np.int8), np.zeros(tiles, np.int8), distance, cand, ctx=dev)
    table = np.zeros(tiles * 640, np.float32)
    table[index] = est
    assert np.array_equal(table.view(np.uint32), s["estimates"].ravel().view(np.uint32)), "the table is not the stand-alone estimate"
    # the field and the masking are the stand-alone entries on the planes before the sharpening
    aq = J.initial_quant_field(s["before"], distance if gab else 0.62 * distance, ctx=dev)[0]
    assert np.array_equal(aq.view(np.uint32), s["aq_map"].view(np.uint32))
    assert np.array_equal(J.masking_1x1(s["before"], ctx=dev).view(np.uint32), s["mask1x1"].view(np.uint32))
    assert np.array_equal(s["before"], s["after"]) == (not gab)
    return model, s


def check_under_own_choices(J, model, size, distance, gab, max_band=1e-3):
    """test_adaptive_quant_f64.check_forward_aq without its comparison of the transform choices (the reading there selects by
    activity): qf, DC and AC by decide() under the model's own acs, tolerances and band caps as there."""
    img = case_image(J, size)
    R = E.Reading(img, aq_header(J, distance), distance=distance, gab=gab, strategy_mode=0)
    acs = model["acs"]
    first = (acs & 1) == 1
    t = qf_reading(R, img, acs, distance, gab)[first]
    got = model["qf"][first]
    amb_q, wrong = E.decide(got, t, E.quant_field_int, A.QF_DELTA_REL * t)
    assert not wrong.any(), "quant field differs at %d first blocks: %s vs reading %s" % (wrong.sum(), got[wrong][:4], t[wrong][:4])
    assert amb_q.sum() <= 0.01 * first.sum(), (int(amb_q.sum()), int(first.sum()))
    assert np.all(model["qf"][~first] == 0)
    dc, co, used = R.transform(acs, model["qf"], dc_y=model["dc"][1], coeffs_y=model["coeffs"][:, 1])
    amb_d, wrong = E.decide(model["dc"], dc, E.round_dc, E.DELTA["dc"])
    assert not wrong.any(), "DC differs at %d of %d" % (wrong.sum(), wrong.size)
    sel = np.broadcast_to(used[:, None, :], co.shape)
    amb_a, wrong = E.decide(model["coeffs"][sel], co[sel], E.quantise_ac, E.DELTA["ac"])
    assert not wrong.any(), "AC differs at %d of %d" % (wrong.sum(), wrong.size)
    assert amb_d.sum() <= max_band * dc.size and amb_a.sum() <= max_band * sel.sum(), (amb_d.sum(), amb_a.sum())
    kinds, counts = np.unique(acs[first] >> 1, return_counts=True)
    cov = {num: (cx, cy) for _, num, cx, cy in W.KINDS}
    by, bx = np.nonzero(first)
    off = sum(1 for y, x in zip(by, bx) if x % cov[int(acs[y, x]) >> 1][0] or y % cov[int(acs[y, x]) >> 1][1])
    print("%dx%d d%.1f gab %d: kinds %s, %d transforms not aligned to their own size; bands qf %d, dc %d, ac %d" % (
        size[0], size[1], distance, gab, dict(zip(kinds.tolist(), counts.tolist())), off, amb_q.sum(), amb_d.sum(), amb_a.sum()))
    return off


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / max(1e-12, np.mean((a.astype(np.float64) - b) ** 2)))


# ---------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,distance,gab", CASES)
def test_cpu_search_is_wired_from_the_stand_alone_entries_and_its_outputs_hold(built, size, distance, gab, mode):
    J = built
    ctx = J.CpuEncContext()
    try:
        model, _ = check_wiring(J, ctx, size, distance, gab, mode)
        plain = J.enc_forward_model(case_image(J, size), None, adaptive_quant=1, acs_search=mode, distance=distance, gab=gab)
        assert all(np.array_equal(model[k], plain[k]) for k in model)  # (with no context: the same model)
    finally:
        ctx.close()
    check_under_own_choices(J, model, size, distance, gab)


def test_the_floating_mode_places_transforms_off_their_own_alignment(built):
    """A condition on the inputs: the 200x136 case is one where mode 2 does what nothing here did before."""
    J = built
    size, distance, gab = CASES[2]
    model = J.enc_forward_model(case_image(J, size), None, adaptive_quant=1, acs_search=2, distance=distance, gab=gab)
    assert check_under_own_choices(J, model, size, distance, gab) > 0


@pytest.mark.parametrize("size,distance,gab", CASES)
def test_streams_decode_with_the_oracle(built, size, distance, gab):
    import jxlo
    J = built
    img = case_image(J, size)
    for mode in (0, 1, 2):
        data = J.encode_rgb8(img, adaptive_quant=1, acs_search=mode, distance=distance, gab=gab)
        o = jxlo.Decoded(data, dumps=False)
        back = o.rgb8
        o.close()
        assert back.shape == img.shape
        print("%dx%d d%.1f gab %d acs_search %d: %d bytes, %.2f dB" % (size[0], size[1], distance, gab, mode, len(data), psnr(back, img)))


def test_parameter_checks_and_the_default(built):
    J = built
    img = J.synth_image(88, 104, seed=4)
    with pytest.raises(J.JxlAmdError):
        J.encode_rgb8(img, acs_search=1)
    with pytest.raises(J.JxlAmdError):
        J.encode_rgb8(img, adaptive_quant=1, acs_search=3)
    with pytest.raises(J.JxlAmdError):
        J.enc_forward_model(img, None, acs_search=2)
    assert J.encode_rgb8(img, adaptive_quant=1, acs_search=0) == J.encode_rgb8(img, adaptive_quant=1)
    assert J.encode_rgb8(img, acs_search=0) == J.encode_rgb8(img)
    ctx = J.CpuEncContext()
    try:
        J.enc_forward_model(img, ctx, adaptive_quant=1)
        with pytest.raises(J.JxlAmdError):
            J.enc_search_debug(ctx)
    finally:
        ctx.close()
