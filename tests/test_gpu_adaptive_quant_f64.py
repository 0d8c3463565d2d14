"""GPU tests (-m gpu): the adaptive quant field kernels (k_enc_aq_cells, k_enc_aq_blocks and the tail of
k_enc_select<true>) against the float64 reading of tests/adaptive_quant_f64.py, with the planes, cases, tolerances and
the decide() rule of test_adaptive_quant_f64.py; the streams of the mode through the three encode routes; and the default
mode's quant field, which shares k_enc_select's tail."""
import numpy as np
import pytest

import adaptive_quant_f64 as A
import enc_fwd_f64 as E
from test_adaptive_quant_f64 import CASES, MOSAIC_KW, _kw, aq_header, case_image, check_entry, check_forward_aq

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", A.KINDS)
def test_device_entry_matches_float64_reading(built, kind):
    J = built
    ctx = J.HipContext()
    try:
        check_entry(J, ctx, kind)
    finally:
        ctx.close()


def test_device_entry_rejects_bad_arguments_and_leaves_the_last_frame(built):
    J = built
    img = J.synth_image(136, 72, seed=3)
    ctx = J.HipContext()
    try:
        with pytest.raises(J.JxlAmdError):
            J.initial_quant_field(np.zeros((3, 12, 8), np.float32), 1.0, ctx=ctx)
        with pytest.raises(J.JxlAmdError):
            J.initial_quant_field(np.zeros((3, 8, 8), np.float32), -1.0, ctx=ctx)
        # a larger field between a forward call and its replay moves the shared buffers: the replay finds them again
        stream = J.encode_rgb8_gpu(img, ctx, adaptive_quant=1)
        J.initial_quant_field(A.crafted("noise", 264, 264), 1.0, ctx=ctx)
        ctx.enc_rerun(1)
        assert ctx.enc_aq_ms() > 0
        assert J.encode_rgb8_gpu(img, ctx, adaptive_quant=1) == stream
    finally:
        ctx.close()


def _both_kernels(J, img, kw, monkeypatch):
    ctx = J.HipContext()
    try:
        tile = J.enc_forward_model(img, ctx, adaptive_quant=1, **kw)
        monkeypatch.setenv("JXLHIP_ENC_BLOCK_KERNEL", "1")
        block = J.enc_forward_model(img, ctx, adaptive_quant=1, **kw)
        monkeypatch.delenv("JXLHIP_ENC_BLOCK_KERNEL")
    finally:
        ctx.close()
    for key in ("acs", "qf", "dc", "coeffs"):
        assert np.array_equal(tile[key], block[key]), "the two transform kernels differ in %s" % key
    return tile


@pytest.mark.parametrize("size,kw", CASES)
def test_forward_kernels_match_float64_reading(built, size, kw, monkeypatch):
    J = built
    img = case_image(J, size)
    model = _both_kernels(J, img, kw, monkeypatch)
    check_forward_aq(model, img, aq_header(J, kw.get("distance", 1.0)), **_kw(kw))


def test_forward_kernels_mosaic_match_float64_reading(built, monkeypatch):
    J = built
    model = _both_kernels(J, E.mosaic(), MOSAIC_KW, monkeypatch)
    assert len(np.unique(model["acs"][(model["acs"] & 1) == 1])) == 12
    check_forward_aq(model, E.mosaic(), aq_header(J, MOSAIC_KW["distance"]), **_kw(MOSAIC_KW))


def test_three_routes_write_one_stream_that_decodes(built):
    import jxlo
    J = built
    img = J.synth_image(520, 300, seed=21)
    ctx = J.HipContext()
    try:
        plain = J.encode_rgb8_gpu(img, ctx, distance=1.0, adaptive_quant=1)
        t1, t2 = {}, {}
        assert J.encode_rgb8_gpu(img, ctx, timings=t1, device_tokens=True, distance=1.0, adaptive_quant=1) == plain
        assert J.encode_rgb8_gpu(img, ctx, timings=t2, device_entropy=True, distance=1.0, adaptive_quant=1) == plain
        assert t1["device_tokens"] > 0 and t2["device_entropy"] > 0
        assert plain != J.encode_rgb8_gpu(img, ctx, distance=1.0)
    finally:
        ctx.close()
    got = J.decode_rgb8(plain)
    want = jxlo.Decoded(plain, dumps=False).rgb8
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert got.shape == want.shape == img.shape and d.max() <= 1, d.max()
    mse = np.mean((want.astype(np.float64) - img) ** 2)
    print("520x300 d1.0 adaptive_quant=1: %d bytes, %.2f dB" % (len(plain), 10 * np.log10(255.0 ** 2 / mse)))


def test_default_mode_quant_field_is_what_it_was(built):
    """adaptive_quant=0 through the same k_enc_select source: the activity rule's field, by check_forward."""
    J = built
    img = J.synth_image(520, 300, seed=531)
    ctx = J.HipContext()
    try:
        model = J.enc_forward_model(img, ctx, adaptive_quant=0, distance=1.0)
        assert all(np.array_equal(model[k], v) for k, v in J.enc_forward_model(img, ctx, distance=1.0).items())
    finally:
        ctx.close()
    E.check_forward(model, img, E.header_scalars(J, 1.0), distance=1.0)
