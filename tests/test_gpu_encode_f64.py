"""GPU tests (-m gpu): the forward VarDCT kernels (jxlhip_enc_forward: k_enc_xyb, the row-form sharpening, k_enc_activity,
k_enc_select, k_enc_offsets and the transform kernels) against the float64 reading of tests/enc_fwd_f64.py, with the
comparison rule of enc_fwd_f64.check_forward. Both transform kernels are run: the 64x64-tile form (the default) and the
one-workgroup-per-transform form (JXLHIP_ENC_BLOCK_KERNEL), which claim the same summation order and must agree bit for
bit."""
import numpy as np
import pytest

import enc_fwd_f64 as E
from test_enc_fwd_f64 import MOSAIC_KW, check_mosaic, _reading_kw

pytestmark = pytest.mark.gpu

# every size listed once at least; together: distances 0.3 / 1 / 4, gab 0 / 1, strategy modes 0 / 1
GPU_CASES = [((8, 8), dict(distance=0.3, gab=0)), ((113, 4), dict(distance=1.0, strategy_mode=0)), ((263, 9), dict(distance=4.0)),
             ((257, 260), dict(distance=1.0, gab=0)), ((257, 260), dict(distance=0.3)), ((520, 300), dict(distance=1.0)),
             ((520, 300), dict(distance=4.0, gab=0, strategy_mode=0)), ((1000, 700), dict(distance=0.3)),
             ((1000, 700), dict(distance=4.0)), ((2048, 1111), dict(distance=1.0)),
             ((2048, 1111), dict(distance=0.3, gab=0, strategy_mode=0)), ((3840, 2160), dict(distance=1.0))]


def _both_kernels(J, img, kw, monkeypatch):
    ctx = J.HipContext()
    try:
        tile = J.enc_forward_model(img, ctx, **kw)
        monkeypatch.setenv("JXLHIP_ENC_BLOCK_KERNEL", "1")
        block = J.enc_forward_model(img, ctx, **kw)
        monkeypatch.delenv("JXLHIP_ENC_BLOCK_KERNEL")
    finally:
        ctx.close()
    return tile, block


@pytest.mark.parametrize("size,kw", GPU_CASES)
def test_forward_kernels_match_float64_reading(built, size, kw, monkeypatch):
    J = built
    img = J.synth_image(size[0], size[1], seed=size[0] + 11)
    header = E.header_scalars(J, kw.get("distance", 1.0))
    tile, block = _both_kernels(J, img, kw, monkeypatch)
    E.check_forward(tile, img, header, **_reading_kw(kw))
    for key in ("acs", "qf", "dc", "coeffs"):
        assert np.array_equal(tile[key], block[key]), "the two transform kernels differ in %s" % key


def test_forward_kernels_every_size_class_match_float64_reading(built, monkeypatch):
    J = built
    tile, block = _both_kernels(J, E.mosaic(), MOSAIC_KW, monkeypatch)
    check_mosaic(J, tile)
    for key in ("acs", "qf", "dc", "coeffs"):
        assert np.array_equal(tile[key], block[key]), "the two transform kernels differ in %s" % key
