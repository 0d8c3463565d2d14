"""GPU tests (-m gpu): the forward path with the reference's AC-strategy search on the device (strategy_mode 2 and 3 of
jxlhip_enc_forward: acs_search 1 and 2), with the cases and checks of test_acs_search.py. The wiring checks are exact and run
against the stand-alone device entries on the same context. The device and the CPU double need not choose the same
transforms (their estimates differ in the last place, and one flipped comparison cascades): the share of blocks that agree is
printed, and nothing is asserted about it."""
import numpy as np
import pytest

from test_acs_search import CASES, MODES, case_image, check_under_own_choices, check_wiring, psnr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built):
    c = built.HipContext()
    yield c
    c.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size,distance,gab", CASES)
def test_device_search_is_wired_from_the_stand_alone_entries_and_its_outputs_hold(built, ctx, size, distance, gab, mode):
    J = built
    model, _ = check_wiring(J, ctx, size, distance, gab, mode)
    check_under_own_choices(J, model, size, distance, gab)
    cpu = J.enc_forward_model(case_image(J, size), None, adaptive_quant=1, acs_search=mode, distance=distance, gab=gab)
    print("device and CPU double choose the same strategy at %.1f %% of the blocks" % (100.0 * np.mean(model["acs"] == cpu["acs"])))


@pytest.mark.parametrize("mode", MODES)
def test_three_routes_write_one_stream_that_decodes(built, mode):
    import jxlo
    J = built
    img = J.synth_image(520, 300, seed=21)
    ctx = J.HipContext()
    try:
        kw = dict(distance=1.0, adaptive_quant=1, acs_search=mode)
        plain = J.encode_rgb8_gpu(img, ctx, **kw)
        t1, t2 = {}, {}
        assert J.encode_rgb8_gpu(img, ctx, timings=t1, device_tokens=True, **kw) == plain
        assert J.encode_rgb8_gpu(img, ctx, timings=t2, device_entropy=True, **kw) == plain
        assert t1["device_tokens"] > 0 and t2["device_entropy"] > 0
        assert plain != J.encode_rgb8_gpu(img, ctx, distance=1.0, adaptive_quant=1)
    finally:
        ctx.close()
    got = J.decode_rgb8(plain)
    want = jxlo.Decoded(plain, dumps=False).rgb8
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert got.shape == want.shape == img.shape and d.max() <= 1, d.max()
    print("520x300 d1.0 adaptive_quant=1 acs_search=%d: %d bytes, %.2f dB" % (mode, len(plain), psnr(want, img)))


def test_rerun_replays_the_mode_and_the_times_are_the_modes_own(built):
    J = built
    img = J.synth_image(520, 300, seed=21)
    ctx = J.HipContext()
    try:
        with pytest.raises(J.JxlAmdError):
            ctx.enc_search_ms()
        model = J.enc_forward_model(img, ctx, adaptive_quant=1, acs_search=2)
        first = J.enc_search_debug(ctx)
        ctx.enc_rerun(2)
        ms = ctx.enc_search_ms()
        print("520x300 acs_search=2: mask1x1 %.3f ms, estimates %.3f ms, walk %.3f ms" % ms)
        assert all(v > 0 for v in ms)
        again = J.enc_search_debug(ctx)
        assert all(np.array_equal(first[k].view(np.uint32), again[k].view(np.uint32)) for k in first)
        J.enc_forward_model(img, ctx, adaptive_quant=1)
        with pytest.raises(J.JxlAmdError):
            ctx.enc_search_ms()
        with pytest.raises(J.JxlAmdError):
            J.enc_search_debug(ctx)
        assert all(np.array_equal(v, J.enc_forward_model(img, ctx, adaptive_quant=1, acs_search=2)[k]) for k, v in model.items())
    finally:
        ctx.close()


def test_the_other_modes_are_untouched_by_a_search_on_the_same_context(built):
    J = built
    img = J.synth_image(520, 300, seed=21)
    ctx = J.HipContext()
    try:
        before = J.encode_rgb8_gpu(img, ctx, adaptive_quant=1)
        plain_before = J.encode_rgb8_gpu(img, ctx)
        J.encode_rgb8_gpu(img, ctx, adaptive_quant=1, acs_search=2)
        assert J.encode_rgb8_gpu(img, ctx, adaptive_quant=1) == before
        assert J.encode_rgb8_gpu(img, ctx) == plain_before
    finally:
        ctx.close()


def test_device_forward_refuses_the_search_without_the_adaptive_field(built):
    J = built
    ctx = J.HipContext()
    try:
        with pytest.raises(J.JxlAmdError):
            J.enc_forward_model(J.synth_image(64, 64, seed=2), ctx, acs_search=1)
    finally:
        ctx.close()
